"""Nearest-x2 upsample + 3x3 convolution as four 2x2 sub-pixel convolutions (conv3x3_halo_kernel, SUB = 1 forward / SUB = 2 input
gradient; include/dvq_hip.h, dvq_conv3x3_subpixel_ok).  Reference: F.interpolate(nearest) + F.conv2d and autograd in fp64 on the
bf16-rounded inputs and the 3x3 weights (bf16-representable masters).  Shapes are the smallest at which each piece can go wrong:

  n2_8x32_64_64      one tile, 64-channel instance (NT = 2), one chunk per class in the input gradient, N = 2: the image stride
  n1_16x64_128_128   2 x 2 tiles: halo rows / columns across tile borders, tile and class offsets of the store, 128-channel instance
                     (NT = 4), two chunks per class: the chunk -> class -> scalar-offset arithmetic
  n1_8x32_64_256     two output-channel blocks per class
  n1_8x16_64_64      NOT eligible (low-res width 16): the 9-tap path, same values

`pytest -m gpu`."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

SHAPES = {"n2_8x32_64_64": (2, 8, 32, 64, 64), "n1_16x64_128_128": (1, 16, 64, 128, 128), "n1_8x32_64_256": (1, 8, 32, 64, 256)}
INELIGIBLE = (1, 8, 16, 64, 64)
_cache = {}


def _bf(t):
    return t.to(torch.bfloat16).to(torch.float64)


def _case(dev, key):
    """inputs, packs and the fp64 reference of one shape, computed once"""
    if key in _cache:
        return _cache[key]
    from dynamicvectorquantization_amd import kernels as K
    n, h, w, cin, cout = SHAPES.get(key, INELIGIBLE)
    gen = torch.Generator().manual_seed(1000 + h * w + cin + cout)
    x = _bf(torch.randn(n, cin, h, w, generator=gen, dtype=torch.float64))
    W = _bf(torch.randn(cout, cin, 3, 3, generator=gen, dtype=torch.float64) / (cin * 9) ** 0.5)
    b = torch.randn(cout, generator=gen, dtype=torch.float64).float().double() * 0.5
    g = _bf(torch.randn(n, cout, 2 * h, 2 * w, generator=gen, dtype=torch.float64))
    xr = x.clone().requires_grad_(True)
    y_lin = F.conv2d(F.interpolate(xr, scale_factor=2, mode="nearest"), W, None, padding=1)
    dx = torch.autograd.grad((y_lin * g).sum(), xr)[0]
    d = K.conv_desc(n, 2 * h, 2 * w, cin, cout, 3, 3, 1, 1, 1, 2 * h, 2 * w, True, torch.bfloat16)
    sub = key in SHAPES
    wbuf, wtbuf = K.pack_weight(W.float().to(dev), cin, cout, torch.bfloat16, subpixel=sub)
    c = dict(n=n, h=h, w=w, cin=cin, cout=cout, d=d, sub=sub, W=W, wbuf=wbuf, wtbuf=wtbuf,
             x=x.permute(0, 2, 3, 1).contiguous().to(dev).to(torch.bfloat16), bias=b.float().to(dev),
             g=g.permute(0, 2, 3, 1).contiguous().to(dev).to(torch.bfloat16),
             y_lin=y_lin.detach().permute(0, 2, 3, 1), y=(y_lin.detach() + b[None, :, None, None]).permute(0, 2, 3, 1),
             dx=dx.permute(0, 2, 3, 1))
    _cache[key] = c
    return c


def _fwd(c, stats=None, bias=True):
    from dynamicvectorquantization_amd import kernels as K
    return K.conv2d_fwd(c["d"], c["x"], c["wbuf"], c["bias"] if bias else None, out_stats=stats, out_groups=32 if stats is not None else 0,
                        subpixel=c["sub"])


def _dgrad(c):
    from dynamicvectorquantization_amd import kernels as K
    return K.conv2d_dgrad(c["d"], c["g"], c["wtbuf"], subpixel=c["sub"])


def _check_stats(y, stats, cout):
    """(sum, sum of squares) of the STORED bf16 output per (n, group): the bound test_gpu_fullsize.py puts on the halo statistics
    (error / (|reference| + 1) < 2e-4); printed as well in the units of profiles/r06_v7_halo_stats_check.txt"""
    n = y.shape[0]
    v = y.double().reshape(n, -1, 32, cout // 32).permute(0, 2, 1, 3).reshape(n, 32, -1)
    ref = torch.stack([v.sum(-1), (v * v).sum(-1)], dim=-1)
    got = stats.double()
    rms, cnt = (ref[..., 1] / v.shape[-1]).sqrt(), v.shape[-1]
    print("stats: sum err / (rms sqrt(count)) %.3e   sum-of-squares rel err %.3e" % (
        float(((got[..., 0] - ref[..., 0]).abs() / (rms * cnt ** 0.5)).max()), float(((got[..., 1] - ref[..., 1]).abs() / ref[..., 1]).max())))
    err = float(((got - ref).abs() / (ref.abs() + 1.0)).max())
    assert err < 2e-4, err


@pytest.mark.parametrize("key", sorted(SHAPES))
def test_forward_values_bias_and_statistics(dev, key):
    """forward with bias and the statistics epilogue; every image border lies in a tile of these shapes"""
    from dynamicvectorquantization_amd import kernels as K
    c = _case(dev, key)
    assert K.conv_subpixel_ok(c["d"])
    K.ensure_workspace(dev)
    stats = torch.zeros(c["n"], 32, 2, dtype=torch.float64, device=dev)
    y = _fwd(c, stats)
    assert y.shape == (c["n"], 2 * c["h"], 2 * c["w"], c["cout"])
    ref = c["y"]
    err = float((y.double().cpu() - ref).abs().max() / ref.abs().max())
    print(f"{key}: forward max err / max|ref| {err:.3e}")
    assert err < 2e-2, err
    _check_stats(y, stats, c["cout"])


@pytest.mark.parametrize("key", sorted(SHAPES))
def test_input_gradient_values_without_workspace(dev, key):
    from dynamicvectorquantization_amd import kernels as K
    c = _case(dev, key)
    ws_bytes = c["n"] * 4 * c["h"] * c["w"] * c["cin"] * 2                # the full-resolution gradient the 9-tap path asks for
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    dx = _dgrad(c)
    torch.cuda.synchronize()
    assert torch.cuda.max_memory_allocated() - before < ws_bytes, "a full-resolution workspace was allocated"
    ref = c["dx"]
    err = float((dx.double().cpu() - ref).abs().max() / ref.abs().max())
    print(f"{key}: input gradient max err / max|ref| {err:.3e}")
    assert err < 3e-2, err
    # the library itself takes no workspace on this path
    d2 = K._with_subpixel(c["d"])
    dx2 = torch.empty_like(dx)
    s = torch.cuda.current_stream().cuda_stream
    rc = K.lib().dvq_conv2d_dgrad(C.byref(d2), c["g"].data_ptr(), c["wtbuf"].data_ptr(), dx2.data_ptr(), None, None, 0, None, 0, s)
    assert rc == 0, K.lib().dvq_last_error()
    assert torch.equal(dx, dx2)


def _adjoint_gap(c, draws=8):
    """rms over `draws` gradients g of |<fwd(x), g> - <x, dgrad(g)>| / (|fwd(x)| |g|): fp64 sums of the device's bf16 outputs, no bias.
    The gap of ONE pair (x, g) is a single draw of a zero-mean sum of output roundings -- on the 9-tap pair it came out 8.1e-8 at one of
    these shapes and 5.6e-6 at another -- so single draws cannot be compared; the rms over independent gradients can."""
    from dynamicvectorquantization_amd import kernels as K
    y = _fwd(c, bias=False).double()
    gen = torch.Generator().manual_seed(77)
    sq = 0.0
    for _ in range(draws):
        g = torch.randn(y.shape, generator=gen).to(torch.bfloat16).to(y.device)
        dx = K.conv2d_dgrad(c["d"], g, c["wtbuf"], subpixel=c["sub"]).double()
        a, b = (y * g.double()).sum(), (c["x"].double() * dx).sum()
        sq += float((a - b).abs() / (y.norm() * g.double().norm())) ** 2
    return (sq / draws) ** 0.5


# _adjoint_gap of the 9-tap pair (upsample = 1: the form this one replaces), measured on an MI355X
ADJOINT_9TAP = {"n2_8x32_64_64": 8.860e-06, "n1_16x64_128_128": 4.542e-06, "n1_8x32_64_256": 4.907e-06}


@pytest.mark.parametrize("key", sorted(SHAPES))
def test_adjoint_identity_with_the_devices_own_forward(dev, key):
    """<fwd(x), g> against <x, dgrad(g)> with the device's own forward; allowed: twice what the 9-tap pair (upsample = 1 forward, 9-tap
    input gradient + 2x2 sum pass) shows at the same shape.  _adjoint_gap measured on an MI355X, 9-tap pair / sub-pixel pair:
      n2_8x32_64_64     8.860e-06 / 5.644e-06
      n1_16x64_128_128  4.542e-06 / 3.239e-06
      n1_8x32_64_256    4.907e-06 / 4.122e-06
    (single (x, g) pairs, the first form of this measurement: 5.609e-06 / 6.747e-06, 1.206e-06 / 4.035e-07, 8.144e-08 / 3.102e-06)"""
    c = _case(dev, key)
    gap = _adjoint_gap(c)
    old = _adjoint_gap(dict(c, sub=False))          # the 9-tap pair reads the 3x3 packs at the head of the same buffers
    print(f"{key}: adjoint gap sub-pixel {gap:.3e}   9-tap {old:.3e}")
    assert gap <= 2 * ADJOINT_9TAP[key], (gap, ADJOINT_9TAP[key])


def test_ineligible_shape_takes_the_nine_tap_path(dev):
    from dynamicvectorquantization_amd import kernels as K
    c = _case(dev, "n1_8x16_64_64")
    assert not K.conv_subpixel_ok(c["d"])
    y, dx = _fwd(c), _dgrad(c)
    assert float((y.double().cpu() - c["y"]).abs().max() / c["y"].abs().max()) < 2e-2
    assert float((dx.double().cpu() - c["dx"]).abs().max() / c["dx"].abs().max()) < 3e-2
    with pytest.raises(Exception):                   # upsample == 2 on a shape the predicate refuses is an error, not a fallback
        K.conv2d_fwd(c["d"], c["x"], c["wbuf"], c["bias"], subpixel=True)


def test_deterministic_mode_bit_equal_and_ordered(dev):
    from dynamicvectorquantization_amd import kernels as K
    c = _case(dev, "n1_16x64_128_128")
    K.ensure_workspace(dev)
    try:
        K.set_deterministic(True)
        c0 = K.unordered_launches()
        outs = []
        for _ in range(2):
            stats = torch.zeros(c["n"], 32, 2, dtype=torch.float64, device=dev)
            outs.append((_fwd(c, stats), stats, _dgrad(c)))
        torch.cuda.synchronize()
        assert K.unordered_launches() == c0, "deterministic mode took an unordered path"
        for a, b in zip(*outs):
            assert torch.equal(a, b)
    finally:
        K.set_deterministic(False)


def test_dispatch_reports_the_halo_family(dev):
    from dynamicvectorquantization_amd import kernels as K
    c = _case(dev, "n2_8x32_64_64")
    K.profile_start(8)
    try:
        _fwd(c)
        _dgrad(c)
    finally:
        prof = K.profile_stop()
    assert set(prof) == {"conv3x3_halo_kernel"} and prof["conv3x3_halo_kernel"]["launches"] == 2, prof


def _torch_subpixel_packs(W):
    """bf16(fp32 sum of the group's taps), rows then columns ascending: Weff [4][Cout][4][Cin], WeffT [Cin][4][4][Cout]"""
    W = W.float()
    cout, cin = W.shape[:2]
    weff = torch.zeros(4, cout, 4, cin, dtype=torch.float32)
    for cls in range(4):
        for t in range(4):
            py, px, a, b = cls >> 1, cls & 1, t >> 1, t & 1
            us = range(1 + py, 3) if a else range(0, py + 1)
            vs = range(1 + px, 3) if b else range(0, px + 1)
            s = torch.zeros(cout, cin, dtype=torch.float32)
            for u in us:
                for v in vs:
                    s = s + W[:, :, u, v]
            weff[cls, :, t] = s
    return weff.to(torch.bfloat16), weff.permute(3, 0, 2, 1).contiguous().to(torch.bfloat16)


def test_weight_packs_multi_equals_single_equals_torch(dev):
    from dynamicvectorquantization_amd import kernels as K
    from dynamicvectorquantization_amd import runtime as rt
    from dynamicvectorquantization_amd.layers import Conv2d
    torch.manual_seed(5)
    mods = [Conv2d(64, 64, 3, 1, 1, upsample=True), Conv2d(128, 64, 3, 1, 1), Conv2d(64, 128, 3, 1, 1, upsample=True),
            Conv2d(40, 72, 3, 1, 1, upsample=True)]
    mods = [m.to(dev) for m in mods]
    with rt.compute_dtype_ctx(torch.bfloat16):
        for m in mods:
            m.packed(torch.bfloat16)
        assert [m._packs[torch.bfloat16]["sub"] for m in mods] == [True, False, True, False]
        with torch.no_grad():
            for m in mods:
                m.weight.add_(torch.randn_like(m.weight))     # the next packed() call repacks all of them in one launch
        for m in mods:
            m.packed(torch.bfloat16)
    for m in mods:
        e = m._packs[torch.bfloat16]
        cin, cout = m.in_channels, m.out_channels
        rw, rwt = K.pack_weight(m.weight.detach(), e["cin_p"], e["cout_p"], torch.bfloat16)      # the plain 3x3 packs
        assert torch.equal(e["w"][:cout], rw) and torch.equal(e["wt"], rwt)
        if not e["sub"]:
            continue
        sw, swt = K.pack_weight(m.weight.detach(), cin, cout, torch.bfloat16, subpixel=True)
        w9, wt9, weff, wefft = K.subpixel_pack_views(sw, swt, cout, cin)
        assert torch.equal(w9, rw) and torch.equal(wt9, rwt)
        n9 = 9 * cout * cin
        mw = e["w"].as_strided((25 * cout * cin,), (1,))        # the module's flat buffers behind its 3x3 views
        mwt = e["wt"].as_strided((25 * cout * cin,), (1,))
        assert torch.equal(mw, sw) and torch.equal(mwt, swt), "multi-tensor pack differs from the single-layer pack"
        tw, twt = _torch_subpixel_packs(m.weight.detach().cpu())
        assert torch.equal(weff.cpu(), tw) and torch.equal(wefft.cpu(), twt)
        assert mw[n9:].numel() == 16 * cout * cin


def test_upsample_module_forward_backward(dev):
    """layers.Upsample(64, True) against the torch module: the wiring of the packs, the input gradient at low resolution and the weight
    gradient, which stays on the 9-tap kernel reading the stored low-resolution input.  Weight / bias gradients: exact bf16 products,
    fp32 accumulation over 2 * 16 * 64 pixels -> 1e-3 of the largest element is generous"""
    from dynamicvectorquantization_amd import layers as L
    from dynamicvectorquantization_amd import runtime as rt
    torch.manual_seed(9)
    mod = L.Upsample(64, True).to(dev)
    with torch.no_grad():
        mod.conv.weight.copy_(mod.conv.weight.to(torch.bfloat16).float())
    x = torch.randn(2, 64, 8, 32).to(torch.bfloat16).float().to(dev).requires_grad_(True)
    gout = torch.randn(2, 64, 16, 64).to(torch.bfloat16).float().to(dev)
    with rt.compute_dtype_ctx(torch.bfloat16):
        y = mod(x)
        assert mod.conv._packs[torch.bfloat16]["sub"]
        (y * gout).sum().backward()
    xr = x.detach().double().cpu().requires_grad_(True)
    Wr = mod.conv.weight.detach().double().cpu().requires_grad_(True)
    br = mod.conv.bias.detach().double().cpu().requires_grad_(True)
    yr = F.conv2d(F.interpolate(xr, scale_factor=2, mode="nearest"), Wr, br, padding=1)
    (yr * gout.double().cpu()).sum().backward()

    def rel(a, b):
        return float((a.double().cpu() - b).abs().max() / b.abs().max())
    assert rel(y.detach(), yr.detach()) < 2e-2
    assert rel(x.grad, xr.grad) < 3e-2
    assert rel(mod.conv.weight.grad, Wr.grad) < 1e-3
    assert rel(mod.conv.bias.grad, br.grad) < 1e-3
