"""tests/vq_math.py (the float64 restatement behind test_gpu_quantiser_kernels.py) against torch float64 -- F.embedding, autograd of the
straight-through + commitment expression, F.avg_pool2d, repeat_interleave + where with autograd, torch.cdist -- to 1e-12 relative, and
against the fixtures the reference made (tests/golden/vq_ema.npz, vq_forward.npz) within the bounds of the GPU tests that use them.
No GPU."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import vq_math as M
from conftest import load_golden
from dynamicvectorquantization_amd import synth

REL = 1e-12


def _close(got, ref, what):
    got, ref = np.asarray(got, dtype=np.float64), ref.detach().numpy() if isinstance(ref, torch.Tensor) else np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, f"{what}: shape {got.shape} against {ref.shape}"
    scale = max(float(np.abs(ref).max()), 1e-300)
    assert float(np.abs(got - ref).max()) <= REL * scale, f"{what}: {float(np.abs(got - ref).max()) / scale:.3e} relative"


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))


def _up(t, r):
    return t.repeat_interleave(r, dim=1).repeat_interleave(r, dim=2)


def test_bf16_round_is_torch_rne():
    rs = np.random.RandomState(1)
    a = np.concatenate([rs.standard_normal(4096).astype(np.float32) * np.float32(10.0) ** rs.randint(-30, 30, 4096).astype(np.float32),
                        np.array([0.0, -0.0, 1.0, 1.00390625, 1.01171875, -1.00390625, np.inf, -np.inf, 3.3895314e38, 1e-40], dtype=np.float32)])
    want = torch.from_numpy(a).to(torch.bfloat16).float().numpy()
    assert np.array_equal(M.bf16_round(a).view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("masked", [False, True], ids=["no-mask", "mask"])
def test_gather_straight_through_loss_backward(masked):
    rs = np.random.RandomState(2)
    n, d, k, beta, c = 37, 13, 11, 0.25, 3.0
    x, e, g = rs.standard_normal((n, d)), rs.standard_normal((k, d)), rs.standard_normal((n, d))
    idx = rs.randint(0, k, n)
    mask = rs.choice([1.0, 0.25, 0.0625, 0.0], n) if masked else None
    xt = _t(x).requires_grad_(True)
    et = F.embedding(torch.from_numpy(idx), _t(e))
    _close(M.gather(e, idx), et, "gather")
    _close(M.gather(e, idx.reshape(1, n, 1)), F.embedding(torch.from_numpy(idx.reshape(1, n, 1)), _t(e)), "gather, 3-d idx")
    m = torch.ones(n, 1, dtype=torch.float64) if mask is None else _t(mask)[:, None]
    xq = xt + (et - xt).detach()
    loss = beta * (m * (xt - et.detach()) ** 2).mean() + (m * (xt.detach() - et) ** 2).mean()
    (c * loss + (xq * _t(g)).sum()).backward()
    _close(M.straight_through(x, e, idx), xq, "straight-through output")
    _close(M.vq_loss(x, e, idx, mask, beta), loss, "loss")
    _close(M.loss_sum(x, e, idx, mask), (m * (xt - et) ** 2).sum(), "loss sum")
    _close(M.backward(g, x, e, idx, mask, c * 2.0 * beta / (n * d)), xt.grad, "backward")
    # the stored value: float32 arithmetic, then one bf16 rounding
    x32, e32 = x.astype(np.float32), e.astype(np.float32)
    t32 = torch.from_numpy(x32) + (torch.from_numpy(e32)[torch.from_numpy(idx)] - torch.from_numpy(x32))
    assert np.array_equal(M.straight_through_f32(x32, e32, idx), t32.numpy())
    assert np.array_equal(M.straight_through_bf16(x32, e32, idx), t32.to(torch.bfloat16).float().numpy())


def test_code_sums_ema_and_normalise():
    rs = np.random.RandomState(3)
    n, d, k, decay, eps = 500, 9, 17, 0.99, 1e-5
    x = rs.standard_normal((n, d))
    idx = rs.randint(0, k - 3, n)                                     # codes k - 3 .. k - 1 own no rows
    sums, cnt = M.code_sums(x, idx, k)
    onehot = F.one_hot(torch.from_numpy(idx), k).double()
    _close(sums, onehot.T @ _t(x), "per-code sums")
    assert np.array_equal(cnt, onehot.sum(0).numpy())
    n0, s0, restart = rs.rand(k) * 300, rs.standard_normal((k, d)), rs.standard_normal((k, d))
    n0[-1], n0[-2], n0[0] = 150.0, 0.7, 0.2                             # without rows: alive, dead; with rows and a small count: dead
    # the reference's expression (quantize2_mask.py:90-105): usage = (n' >= 1), blend, then normalise
    nt = _t(n0) * decay + _t(cnt) * (1 - decay)
    st = _t(s0) * decay + _t(sums) * (1 - decay)
    n1, s1, dead = M.ema_update(n0, s0, cnt, sums, decay)
    _close(n1, nt, "n_ema without restart")
    _close(s1, st, "s_ema without restart")
    assert not dead.any()
    usage = (nt >= 1).double()
    st2 = st * usage[:, None] + _t(restart) * (1 - usage)[:, None]
    nt2 = nt * usage + (1 - usage)
    n2, s2, dead = M.ema_update(n0, s0, cnt, sums, decay, restart)
    _close(n2, nt2, "n_ema with restart")
    _close(s2, st2, "s_ema with restart")
    assert np.array_equal(dead, (usage == 0).numpy()) and 0 < dead.sum() < k
    tot = nt2.sum()
    _close(M.ema_normalize(n2, s2, eps), st2 / (tot * (nt2 + eps) / (tot + k * eps))[:, None], "weight")
    # a NaN count is dead (not >= 1)
    assert M.ema_update([np.nan], np.zeros((1, d)), [0.0], np.zeros((1, d)), 0.5, np.ones((1, d)))[2][0]


def test_distances():
    rs = np.random.RandomState(4)
    x, e = rs.standard_normal((19, 33)), rs.standard_normal((7, 33))
    _close(M.distances(x, e), torch.cdist(_t(x), _t(e)) ** 2, "distances")


@pytest.mark.parametrize("k", [1, 2, 4])
def test_avgpool_and_backward(k):
    rs = np.random.RandomState(5 + k)
    x = rs.standard_normal((2, 3 * k, 5 * k, 8))
    xt = _t(x).requires_grad_(True)
    y = F.avg_pool2d(xt.permute(0, 3, 1, 2), k).permute(0, 2, 3, 1)
    _close(M.avgpool(x, k), y, "pool")
    g = rs.standard_normal(y.shape)
    y.backward(_t(g))
    _close(M.avgpool_bwd(g, k), xt.grad, "pool backward")


def test_dual_merge_and_backward():
    rs = np.random.RandomState(8)
    b, h, w, c = 2, 3, 5, 8
    hf, hc = rs.standard_normal((b, 2 * h, 2 * w, c)), rs.standard_normal((b, h, w, c))
    grain = rs.choice([0, 1, 2, -1], (b, h, w))
    ft, ct = _t(hf).requires_grad_(True), _t(hc).requires_grad_(True)
    fine = _up(torch.from_numpy(grain) != 0, 2)
    merged = torch.where(fine[..., None], ft, _up(ct, 2))
    out, mask = M.dual_merge(hf, hc, grain)
    _close(out, merged, "dual merge")
    assert np.array_equal(mask, torch.where(fine, 1.0, 0.25).numpy())
    g = rs.standard_normal(hf.shape)
    merged.backward(_t(g))
    gf, gc = M.dual_merge_bwd(g, grain)
    _close(gf, ft.grad, "dual merge: fine gradient")
    _close(gc, ct.grad, "dual merge: coarse gradient")
    g32 = g.astype(np.float32)
    got = M.dual_merge_bwd_coarse_f32(g32, grain)
    assert got.dtype == np.float32 and float(np.abs(got - M.dual_merge_bwd(g32, grain)[1]).max()) <= 4 * 2.0 ** -24 * float(np.abs(g32).max()) * 4


@pytest.mark.parametrize("s", [2, 3])
@pytest.mark.parametrize("scaled", [False, True], ids=["no-scale", "scale"])
def test_grain_merge_and_backward(s, scaled):
    rs = np.random.RandomState(9 + s)
    n, hc, wc, c = 2, 3, 5, 8
    heads = [rs.standard_normal((n, hc << l, wc << l, c)) for l in range(s)]
    idx = rs.randint(0, s, (n, hc, wc))
    scale = rs.rand(n, hc, wc) + 0.5 if scaled else None
    f = 1 << (s - 1)
    hs = [_t(h).requires_grad_(True) for h in heads]
    sc = _t(scale).requires_grad_(True) if scaled else None
    lvl = _up(torch.from_numpy(idx), f)
    merged = hs[s - 1]
    for l in range(s - 1):
        merged = torch.where((lvl == l)[..., None], _up(hs[l], 1 << (s - 1 - l)), merged)
    plain = merged
    if scaled:
        merged = merged * _up(sc, f)[..., None]
    out, mask = M.grain_merge(heads, idx, scale)
    _close(out, merged, "merge")
    assert np.array_equal(mask, (4.0 ** -(s - 1 - lvl).double()).numpy())
    g = rs.standard_normal(out.shape)
    merged.backward(_t(g))
    dheads, dscale, mag = M.grain_merge_bwd(g, heads, idx, scale)
    for l in range(s):
        _close(dheads[l], hs[l].grad, f"merge: gradient of level {l}")
    want = (_t(g) * plain.detach()).reshape(n, hc, f, wc, f, c).sum(dim=(2, 4, 5))
    _close(dscale, sc.grad if scaled else want, "merge: dscale")
    assert bool((mag >= np.abs(dscale) * (1 - 1e-12)).all())


# ---- the fixtures the reference made ------------------------------------------------------------------------------------------------------
def test_ema_restatement_reproduces_the_reference_fixture():
    """inputs as test_vq_ema_golden builds them; its bounds (n_ema rtol 1e-5 / atol 1e-6, s_ema and weight rtol 1e-4 / atol 1e-5)"""
    g = load_golden("vq_ema")
    decay, eps = 0.99, 1e-5
    for tag, dead in (("live", False), ("dead", True)):
        n, d, k = (int(v) for v in g[f"{tag}_meta"])
        w = synth.det_param(f"ema.{tag}.w", (k + 1, d)) * 3.0
        x = synth.det_param(f"ema.{tag}.x", (n, d)) * (1.5 if dead else 3.0)
        n0, idx, perm = g[f"{tag}_n_ema0"], g[f"{tag}_idx"], g[f"{tag}_perm"]
        s0 = w[:-1] * n0[:, None]
        sums, cnt = M.code_sums(x, idx, k)
        n1, s1, died = M.ema_update(n0, s0, cnt, sums, decay, M.gather(x, perm[:k]))
        assert bool(died.any()) == dead
        np.testing.assert_allclose(n1, g[f"{tag}_n_ema"], rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(s1, g[f"{tag}_s_ema"], rtol=1e-4, atol=1e-5)
        np.testing.assert_allclose(M.ema_normalize(n1, s1, eps), g[f"{tag}_weight"], rtol=1e-4, atol=1e-5)


def test_forward_restatement_reproduces_the_reference_fixture():
    """x_q, loss and dx of vq_forward.npz from its idx; the bounds of test_vq_forward_golden (atol 1e-6; rtol 1e-5; rtol 1e-5 / atol 1e-6)"""
    g = load_golden("vq_forward")
    beta = 0.25
    for tag in ("a", "b"):
        b, d, h, k, use_mask = (int(v) for v in g[f"{tag}_meta"])
        w = synth.det_param(f"vqfwd.{tag}.codebook", (k + 1, d)) * 4.0
        x = synth.det_param(f"vqfwd.{tag}.x", (b, d, h, h)) * 6.0
        gout = synth.det_param(f"vqfwd.{tag}.gout", x.shape)
        rows = lambda a: np.ascontiguousarray(np.asarray(a).transpose(0, 2, 3, 1)).reshape(-1, d)
        xf, gf, idx = rows(x).astype(np.float32), rows(gout), g[f"{tag}_idx"].reshape(-1)
        mask = g[f"{tag}_mask"].reshape(-1) if use_mask else None
        e = w[:-1].astype(np.float32)
        np.testing.assert_allclose(M.straight_through_f32(xf, e, idx), rows(g[f"{tag}_x_q"]), atol=1e-6)
        np.testing.assert_allclose(M.straight_through(xf, e, idx), rows(g[f"{tag}_x_q"]), atol=1e-6)
        np.testing.assert_allclose(M.vq_loss(xf, e, idx, mask, beta), float(g[f"{tag}_loss"]), rtol=1e-5)
        # the test's objective is 3 loss + sum(x_q gout): dx = gout + 3 (2 beta / numel) mask (x - e)
        np.testing.assert_allclose(M.backward(gf, xf, e, idx, mask, 3.0 * 2.0 * beta / xf.size), rows(g[f"{tag}_dx"]), rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(M.gather(e, g[f"{tag}_idx"]), g[f"{tag}_entry"])
