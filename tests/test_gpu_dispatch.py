"""What the library says about its own dispatch: the kernel family a conv call landed on (dvq_last_kernel, read by kernels._timed while
profiling) and the eligibility predicates against the entry points they speak for.  `pytest -m gpu`.

One bf16, impl 0 case per branch of the conv entry points that notes a family and is reachable with the default environment, each at
the smallest shape that meets the branch's conditions in csrc/igemm.hip, csrc/igemm_nt.hip, csrc/igemm_tn.hip / csrc/conv_halo.hip; the
fp32x3 launch-level routes (route labels "conv_x3_halo" / "conv_wgrad_x3_planes") with their scratch contract.  Noted branches WITHOUT a
case here:
  * gemm_nt_wide_kernel, igemm_nt_kernel: plain GEMMs at K >= 8192 / impl 3 only -- no conv call reaches them with impl 0;
  * gemm_tn_8phase_kernel, gemm_tn_wide_pipe_kernel: no conv call reaches them (gemm_tn calls do by default, under the fixed label
    "gemm_tn");
The activation epilogue of the forward and the activation mask of the input gradient are arguments of the one entry per pass: one
halo case each, and the forward's refusal of an activation together with a residual."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

BF16, F32 = torch.bfloat16, torch.float32


def _desc(K, n, h, w, cin, cout, k, stride=1, pad=None, oh=None, ow=None, dtype=BF16):
    pad = (k - 1) // 2 if pad is None else pad
    oh = (h + 2 * pad - k) // stride + 1 if oh is None else oh
    ow = (w + 2 * pad - k) // stride + 1 if ow is None else ow
    return K.conv_desc(n, h, w, cin, cout, k, k, stride, pad, pad, oh, ow, False, dtype, 0)


def _rand(dev, dtype, *shape):
    return (torch.rand(*shape, device=dev) - 0.5).to(dtype)


def _fwd(K, dev, d, dtype=BF16):
    x, w = _rand(dev, dtype, d.N, d.H, d.W, d.Cin), _rand(dev, dtype, d.Cout, d.KH, d.KW, d.Cin)
    return K.conv2d_fwd(d, x, w, torch.zeros(d.Cout, device=dev))


def _fwd_lrelu(K, dev, d, dtype=BF16):
    x, w = _rand(dev, dtype, d.N, d.H, d.W, d.Cin), _rand(dev, dtype, d.Cout, d.KH, d.KW, d.Cin)
    return K.conv2d_fwd(d, x, w, torch.zeros(d.Cout, device=dev), act=K.ACT_LRELU)


def _dgrad(K, dev, d, dtype=BF16):
    dy, wt = _rand(dev, dtype, d.N, d.OH, d.OW, d.Cout), _rand(dev, dtype, d.Cin, d.KH, d.KW, d.Cout)
    return K.conv2d_dgrad(d, dy, wt)


def _dgrad_relu_mask(K, dev, d, dtype=BF16):
    dy, wt = _rand(dev, dtype, d.N, d.OH, d.OW, d.Cout), _rand(dev, dtype, d.Cin, d.KH, d.KW, d.Cout)
    return K.conv2d_dgrad(d, dy, wt, mask=_rand(dev, dtype, d.N, d.H, d.W, d.Cin), mask_act=K.ACT_RELU)


def _wgrad(K, dev, d, dtype=BF16):
    x, dy = _rand(dev, dtype, d.N, d.H, d.W, d.Cin), _rand(dev, dtype, d.N, d.OH, d.OW, d.Cout)
    dw = torch.zeros(d.Cout, d.Cin, d.KH, d.KW, device=dev)
    K.conv2d_wgrad_oihw(d, x, dy, d.Cin, d.Cout, dw, torch.zeros(d.Cout, device=dev))
    return dw


X3_GEO = dict(n=1, h=8, w=32, cin=64, cout=64, k=3)      # the smallest shape the fp32x3 halo route takes

# (id, pass, family, descriptor arguments of _desc, dtype, compute mode of rt.compute_dtype_ctx, environment switches)
DISPATCH_CASES = [
    # halo_try_impl: H % 8, W % 32, Cin % 64, Cout % 8
    ("halo-fwd", _fwd, "conv3x3_halo_kernel", dict(n=1, h=8, w=32, cin=64, cout=64, k=3), BF16, "bf16", {}),
    # the same entry with an activation epilogue / the input gradient gated through an activation's output: the same kernel
    ("halo-fwd-lrelu", _fwd_lrelu, "conv3x3_halo_kernel", dict(n=1, h=8, w=32, cin=64, cout=64, k=3), BF16, "bf16", {}),
    ("halo-dgrad-relu-mask", _dgrad_relu_mask, "conv3x3_halo_kernel", dict(n=1, h=8, w=32, cin=64, cout=64, k=3), BF16, "bf16", {}),
    # dvq_conv2d_fwd: Cin == 8 (image heads) -> dvq_conv3x3_thin_k_try: W % 32, Cout % 8
    ("thin-k-fwd", _fwd, "conv3x3_thin_k_kernel", dict(n=1, h=8, w=32, cin=8, cout=64, k=3), BF16, "bf16", {}),
    # dvq_conv2d_dgrad: Cout == 8 (gradient of the 3-channel output conv), the same kernel with the taps reversed
    ("thin-k-dgrad", _dgrad, "conv3x3_thin_k_kernel", dict(n=1, h=8, w=32, cin=64, cout=8, k=3), BF16, "bf16", {}),
    # dvq_conv2d_dgrad: 4 x 4 / stride 2 / pad 1, Cin == 8, H == 2 OH (input gradient of the PatchGAN's first conv)
    ("tconv4x4s2-thin", _dgrad, "tconv4x4s2_thin_kernel", dict(n=1, h=16, w=16, cin=8, cout=64, k=4, stride=2, pad=1), BF16, "bf16", {}),
    # launch_nt pipe_ok: 64-channel K slabs, stride 1 / 2; the encoder's downsampling conv (3 x 3 / stride 2, pad bottom / right only)
    ("nt-pipe-down", _fwd, "conv_nt_pipe_kernel", dict(n=1, h=16, w=16, cin=64, cout=64, k=3, stride=2, pad=0, oh=8, ow=8), BF16, "bf16", {}),
    # Cin % 64 != 0: neither the halo nor the pipelined kernel; M * Ncols >= 1024 -> the 128 x 128 LDS-DMA kernel
    ("nt-glds", _fwd, "igemm_nt_glds_kernel", dict(n=1, h=8, w=32, cin=32, cout=32, k=3), BF16, "bf16", {}),
    # 1 x 1 as a plain GEMM on 256 x 256 tiles from 128 workgroups on: ceil(M / 256) * ceil(256 / 256) >= 128 <=> M >= 32513 = 533 x 61
    ("nt-wide-pipe", _fwd, "gemm_nt_wide_pipe_kernel", dict(n=1, h=533, w=61, cin=64, cout=256, k=1), BF16, "bf16", {}),
    # ... and on the 8-phase kernel from K >= 4096 over >= 512 tiles on: 8192 x 4096 x 4096
    ("nt-8phase", _fwd, "gemm_nt_8phase_kernel", dict(n=1, h=64, w=128, cin=4096, cout=4096, k=1), BF16, "bf16", {}),
    # M * Ncols < 1024: no MFMA tile
    ("nt-naive", _fwd, "naive_nt_kernel", dict(n=1, h=4, w=4, cin=8, cout=8, k=1), BF16, "bf16", {}),
    # halo_wgrad_impl: H % 4, W % 32, Cin % 64, Cout % 8
    ("halo-wgrad", _wgrad, "conv3x3_halo_wgrad_kernel", dict(n=1, h=8, w=32, cin=64, cout=64, k=3), BF16, "bf16", {}),
    # launch_tn: a conv off the halo shapes, I % 8 == 0 and J % 8 == 0 -> 8 x 8 pixel patches (1 x 1 convs included)
    ("tn-patch", _wgrad, "conv_tn_patch_kernel", dict(n=2, h=20, w=24, cin=128, cout=64, k=1), BF16, "bf16", {}),
    # launch_tn thin: J == 8 with 1 < taps <= 16 (taps folded into the column tile); Mred >= 256 for the MFMA path
    ("tn-tr-thin", _wgrad, "igemm_tn_tr_kernel", dict(n=1, h=8, w=32, cin=8, cout=64, k=3), BF16, "bf16", {}),
    # Mred < 256: no MFMA tile
    ("tn-naive", _wgrad, "naive_tn_kernel", dict(n=1, h=4, w=4, cin=8, cout=8, k=1), BF16, "bf16", {}),
    # fp32 operands: every forward off the fp32x3 halo shapes is igemm_nt_glds_kernel<float>
    ("fp32-fwd", _fwd, "igemm_nt_glds_kernel", dict(n=1, h=8, w=32, cin=32, cout=32, k=3), F32, "fp32", {}),
    # fp32x3 (dvq_set_fp32_split): the launch-level routes report their route labels; x3_halo_shape_ok: H % 8, W % 32, streamed channels % 64,
    # produced channels % 4
    ("x3-halo-fwd", _fwd, "conv_x3_halo", X3_GEO, F32, "fp32x3", {}),
    ("x3-halo-dgrad", _dgrad, "conv_x3_halo", X3_GEO, F32, "fp32x3", {}),
    ("x3-halo-fwd-thin", _fwd, "conv_x3_halo", dict(X3_GEO, cout=4), F32, "fp32x3", {}),
    # the weight gradient on bf16 planes: one halo-planes launch on the halo shape, three launches of the bf16 path off it -- one record
    ("x3-wgrad-planes-halo", _wgrad, "conv_wgrad_x3_planes", X3_GEO, F32, "fp32x3", {}),
    ("x3-wgrad-planes-3-launches", _wgrad, "conv_wgrad_x3_planes", dict(n=2, h=20, w=24, cin=128, cout=64, k=1), F32, "fp32x3", {}),
    # Cin % 64 != 0: no launch-level route, the in-kernel split of the fp32 kernel
    ("x3-fwd-ineligible", _fwd, "igemm_nt_glds_kernel", dict(n=1, h=8, w=32, cin=32, cout=32, k=3), F32, "fp32x3", {}),
    # the switches at "0" pass no scratch: the families read for these calls, with the switch at "0", on the commit before the library
    # routed fp32x3 itself (ABI 123)
    ("x3-halo-fwd-switch-off", _fwd, "igemm_nt_glds_kernel", X3_GEO, F32, "fp32x3", {"DVQ_X3_HALO": "0"}),
    ("x3-wgrad-switch-off", _wgrad, "igemm_tn_kernel", X3_GEO, F32, "fp32x3", {"DVQ_X3_WGRAD_PLANES": "0"}),
]


@pytest.mark.parametrize("case", DISPATCH_CASES, ids=lambda c: c[0])
def test_dispatch_label(dev, case, monkeypatch):
    from dynamicvectorquantization_amd import kernels as K
    from dynamicvectorquantization_amd import runtime as rt
    _, run, family, geo, dtype, mode, env = case
    for name, value in env.items():
        monkeypatch.setenv(name, value)
    d = _desc(K, dtype=dtype, **geo)
    torch.manual_seed(0)
    with rt.compute_dtype_ctx(mode):
        K.profile_start(8)
        try:
            out = run(K, dev, d, dtype)
        finally:
            fams = K.profile_stop()
    assert list(fams) == [family] and fams[family]["launches"] == 1, fams
    assert bool(torch.isfinite(out.float()).all())


def test_fwd_refuses_activation_with_residual_before_dispatch(dev):
    """act != ACT_NONE excludes a residual: DVQ_EINVAL from the argument check, no kernel family noted"""
    from dynamicvectorquantization_amd import _lib
    from dynamicvectorquantization_amd import kernels as K
    d = _desc(K, n=1, h=8, w=32, cin=64, cout=64, k=3)
    x, w = _rand(dev, BF16, d.N, d.H, d.W, d.Cin), _rand(dev, BF16, d.Cout, d.KH, d.KW, d.Cin)
    r = _rand(dev, BF16, d.N, d.OH, d.OW, d.Cout)
    _fwd(K, dev, d)                     # a call that notes a family first: the refusal below must clear it
    assert K.lib().dvq_last_kernel() == b"conv3x3_halo_kernel"
    with pytest.raises(_lib.DvqError, match="code -1"):
        K.conv2d_fwd(d, x, w, torch.zeros(d.Cout, device=dev), residual=r, act=K.ACT_RELU)
    assert K.lib().dvq_last_kernel() == b""


def test_scratch_query_names_the_launch_level_routes(dev):
    """dvq_conv2d_scratch_bytes: non-zero exactly where a launch-level fp32x3 route exists -- F32 operands, the split on, impl AUTO and,
    for the forward / input gradient, a shape the halo route takes"""
    from dynamicvectorquantization_amd import _lib
    from dynamicvectorquantization_amd import kernels as K
    from dynamicvectorquantization_amd import runtime as rt
    passes = (K.PASS_FWD, K.PASS_DGRAD, K.PASS_WGRAD)
    f32 = _desc(K, dtype=F32, **X3_GEO)
    mfma = _desc(K, dtype=F32, **X3_GEO)
    mfma.impl = _lib.IMPL_MFMA
    with rt.compute_dtype_ctx("fp32x3"):
        assert all(K.conv_scratch_bytes(f32, p) > 0 for p in passes)
        assert all(K.conv_scratch_bytes(_desc(K, dtype=BF16, **X3_GEO), p) == 0 for p in passes)
        assert all(K.conv_scratch_bytes(mfma, p) == 0 for p in passes)
        assert K.conv_scratch_bytes(_desc(K, dtype=F32, **dict(X3_GEO, cin=32)), K.PASS_FWD) == 0
        rt.set_fp32_split(False)              # (the block restores the flag on its way out)
        assert not rt.fp32_split() and all(K.conv_scratch_bytes(f32, p) == 0 for p in passes)


def _x3_operands(K, dev):
    d = _desc(K, dtype=F32, **X3_GEO)
    torch.manual_seed(0)
    t = dict(x=_rand(dev, F32, d.N, d.H, d.W, d.Cin), w=_rand(dev, F32, d.Cout, d.KH, d.KW, d.Cin), bias=_rand(dev, F32, d.Cout),
             dy=_rand(dev, F32, d.N, d.OH, d.OW, d.Cout), wt=_rand(dev, F32, d.Cin, d.KH, d.KW, d.Cout))
    return d, t


def _raw_call(K, d, t, pass_, out, scratch, scratch_bytes):
    """the entry point of `pass_` itself, with the scratch arguments as given"""
    p = lambda v: None if v is None else C.c_void_p(v if isinstance(v, int) else v.data_ptr())
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    if pass_ == K.PASS_FWD:
        return K.lib().dvq_conv2d_fwd(C.byref(d), p(t["x"]), p(t["w"]), p(t["bias"]), None, p(out), None, None, 0, K.ACT_NONE,
                                      p(scratch), scratch_bytes, s), "dvq_conv2d_fwd"
    if pass_ == K.PASS_DGRAD:
        return K.lib().dvq_conv2d_dgrad(C.byref(d), p(t["dy"]), p(t["wt"]), p(out), None, None, K.ACT_NONE, p(scratch), scratch_bytes,
                                        s), "dvq_conv2d_dgrad"
    return K.lib().dvq_conv2d_wgrad(C.byref(d), p(t["x"]), p(t["dy"]), d.Cin, d.Cout, p(out), None, 0, None, p(scratch), scratch_bytes,
                                    s), "dvq_conv2d_wgrad"


def test_null_scratch_is_the_route_without_scratch(dev, monkeypatch):
    """fp32x3 with scratch == NULL is a legal call: the in-kernel split, the very call the host layer makes with DVQ_X3_HALO=0 (both
    kernels write every output element once: equality is exact)"""
    from dynamicvectorquantization_amd import _lib
    from dynamicvectorquantization_amd import kernels as K
    from dynamicvectorquantization_amd import runtime as rt
    d, t = _x3_operands(K, dev)
    with rt.compute_dtype_ctx("fp32x3"):
        monkeypatch.setenv("DVQ_X3_HALO", "0")
        ref = {K.PASS_FWD: K.conv2d_fwd(d, t["x"], t["w"], t["bias"]), K.PASS_DGRAD: K.conv2d_dgrad(d, t["dy"], t["wt"])}
        for pass_, r in ref.items():
            assert K.conv_scratch_bytes(d, pass_) > 0
            out = torch.full_like(r, float("nan"))
            rc, what = _raw_call(K, d, t, pass_, out, None, 0)
            _lib.check(rc, what)
            assert K.lib().dvq_last_kernel() not in (b"", b"conv_x3_halo")
            assert torch.equal(out, r), what


@pytest.mark.parametrize("bad", ["one-byte-short", "misaligned"])
def test_bad_scratch_is_refused_before_any_launch(dev, bad):
    """a non-NULL scratch below dvq_conv2d_scratch_bytes, or not 16-byte aligned: DVQ_EWORKSPACE (-5) from the argument check -- no
    kernel family noted, the output untouched"""
    from dynamicvectorquantization_amd import _lib
    from dynamicvectorquantization_amd import kernels as K
    from dynamicvectorquantization_amd import runtime as rt
    d, t = _x3_operands(K, dev)
    outs = {K.PASS_FWD: (d.N, d.OH, d.OW, d.Cout), K.PASS_DGRAD: (d.N, d.H, d.W, d.Cin), K.PASS_WGRAD: (d.Cout, d.Cin, d.KH, d.KW)}
    with rt.compute_dtype_ctx("fp32x3"):
        for pass_, shape in outs.items():
            need = K.conv_scratch_bytes(d, pass_)
            assert need > 0
            buf = torch.empty(need + 16, dtype=torch.uint8, device=dev)
            assert buf.data_ptr() % 16 == 0
            scratch, nbytes = (buf.data_ptr(), need - 1) if bad == "one-byte-short" else (buf.data_ptr() + 8, need)
            out = torch.full(shape, 7.0, device=dev)
            _fwd(K, dev, _desc(K, **X3_GEO))          # a call that notes a family first: the refusal below must clear it
            assert K.lib().dvq_last_kernel() == b"conv3x3_halo_kernel"
            rc, what = _raw_call(K, d, t, pass_, out, scratch, nbytes)
            with pytest.raises(_lib.DvqError, match="code -5"):
                _lib.check(rc, what)
            assert K.lib().dvq_last_kernel() == b""
            assert bool((out == 7.0).all()), what


@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("hs", [32, 64])
@pytest.mark.parametrize("t", [8, 12])
def test_attn_causal_ok_is_what_the_entry_point_accepts(dev, t, hs, dtype):
    from dynamicvectorquantization_amd import _lib
    from dynamicvectorquantization_amd import kernels as K
    q, k, v = (_rand(dev, dtype, t, hs) for _ in range(3))
    try:
        out, _ = K.attn_causal_fwd(q, k, v, 1, t, 1, hs ** -0.5)
        accepted = True
    except _lib.DvqError:
        accepted = False
    assert K.attn_causal_ok(q, 1, 1, t) == accepted
    assert accepted == (t == 8 and hs == 64 and dtype == BF16)
    if accepted:
        assert bool(torch.isfinite(out.float()).all())


@pytest.mark.parametrize("c", [128, 256])
@pytest.mark.parametrize("t", [32, 40])
def test_attn_full_ok_is_what_the_entry_point_accepts(dev, t, c):
    from dynamicvectorquantization_amd import _lib
    from dynamicvectorquantization_amd import kernels as K
    q, k, v = (_rand(dev, BF16, t, c) for _ in range(3))
    try:
        out, _ = K.attn_full_fwd(q, k, v, 1, t, c ** -0.5)
        accepted = True
    except _lib.DvqError:
        accepted = False
    assert K.attn_full_ok(q, t) == accepted
    assert accepted == (t == 32 and c == 256)
    if accepted:
        assert bool(torch.isfinite(out.float()).all())
