"""Thin tensor-level wrappers over the C ABI (no autograd here).

Every function takes/returns torch tensors living on a HIP device, passes raw device pointers and
the current stream to libdvq_hip.so and never synchronises.  Activations are NHWC contiguous
([N,H,W,C]); `dt(t)` maps torch dtypes to DVQ_F32 / DVQ_BF16.  torch is used for memory and streams
only -- a CPU tensor raises.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib
from . import runtime as rt
from ._lib import ConvDesc, check

_DT = {torch.float32: _lib.F32, torch.bfloat16: _lib.BF16}


def dt(t) -> int:
    d = t if isinstance(t, torch.dtype) else t.dtype
    if d not in _DT:
        raise TypeError(f"unsupported dtype {d}; libdvq_hip computes in float32 or bfloat16")
    return _DT[d]


def vec(dtype) -> int:
    """channel granularity of the MFMA path (elements per 16 bytes)"""
    return 4 if dtype == torch.float32 else 8


def _p(t):
    if t is None:
        return None
    if not t.is_cuda:
        raise _lib.DvqError("libdvq_hip kernels need device tensors (no CPU fallback)")
    if not t.is_contiguous():
        raise _lib.DvqError("libdvq_hip kernels need contiguous tensors")
    return C.c_void_p(t.data_ptr())


def _praw(t):
    """device pointer of a tensor whose physical layout the caller vouches for (e.g. channel-last weight views)"""
    if t is None:
        return None
    if not t.is_cuda:
        raise _lib.DvqError("libdvq_hip kernels need device tensors (no CPU fallback)")
    return C.c_void_p(t.data_ptr())


def is_ohwi(t) -> bool:
    """True if a [Cout,Cin,KH,KW]-shaped tensor is physically stored [Cout][KH][KW][Cin] (FlatParams storage);
    False if it is torch-contiguous.  1x1 kernels are both: reported as contiguous."""
    if t.is_contiguous():
        return False
    co, ci, kh, kw = t.shape
    if t.stride() == (kh * kw * ci, 1, kw * ci, ci):
        return True
    raise _lib.DvqError(f"unsupported weight strides {t.stride()} for shape {tuple(t.shape)}")


_det = [None]         # the library's deterministic flag as last seen here (None: not asked yet; DVQ_DETERMINISTIC=1 sets it at load)


def _s():
    if _det[0] is not False:
        # deterministic mode: the ordered forms keep their per-split partials in the registered workspace
        if _det[0] is None:
            _det[0] = bool(lib().dvq_deterministic())
        if _det[0]:
            ensure_workspace(torch.device("cuda", torch.cuda.current_device()))
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def lib():
    return _lib.load()


# ---------------------------------------------------------------------------------------------
# optional per-kernel-family timing with HIP events on the launch stream (bench.py roofline)
# ---------------------------------------------------------------------------------------------
_prof = None          # {family: [(start_event, end_event, flops, bytes), ...]} while profiling
_pool = []            # pre-created timing events (hipEventCreate is slow on some hosts: never create in the timed region)
_count = None         # launch counter (sizing pass)


def profiling_active() -> bool:
    """True while per-launch HIP-event timing or launch counting is on (such a step must run eagerly, not as a graph replay)"""
    return _prof is not None or _count is not None


def profile_count_start():
    """count timed launches without recording anything (used to size the event pool)"""
    global _count
    _count = 0


def profile_count_stop() -> int:
    global _count
    n, _count = _count or 0, None
    return n


def profile_prepare(max_launches):
    """create `max_launches` timing-event pairs (slow on some hosts: do it outside any timed region)"""
    global _pool
    _pool = [torch.cuda.Event(enable_timing=True) for _ in range(2 * max_launches)]
    for ev in _pool:          # torch creates the HIP event lazily at the first record(): force that now
        ev.record()
    torch.cuda.synchronize()


def profile_start(max_launches=0):
    """start recording with the prepared event pool (or create one now)"""
    global _prof
    if max_launches:
        profile_prepare(max_launches)
    _prof = {}


def profile_stop():
    """-> {family: dict(launches, ms, flops, bytes)}; synchronises."""
    global _prof, _pool
    p, _prof = _prof, None
    _pool = []
    torch.cuda.synchronize()
    out = {}
    for name, recs in (p or {}).items():
        out[name] = dict(launches=len(recs), ms=sum(s.elapsed_time(e) for s, e, _, _ in recs),
                         flops=sum(r[2] for r in recs), bytes=sum(r[3] for r in recs))
    return out


_cur_tag = [None]


def _shape_tags() -> bool:
    """debug: split the families by call geometry"""
    return rt.switch("DVQ_PROFILE_SHAPES") == "1"


def _tag(d, mode):
    if _shape_tags():
        _cur_tag[0] = f"{mode} N{d.N} {d.H}x{d.W} {d.Cin}->{d.Cout} k{d.KH}s{d.stride}{'u' if d.upsample else ''}"


def _timed(name, flops, nbytes, fn, entry=None):
    """name=None (_timed_conv): the record is keyed by the kernel family the library noted at the dispatch branch the call took
    (dvq_last_kernel), or by `entry`, the entry point's name, when it noted none -- a branch without a note shows up in the table"""
    global _count
    tag = None
    if _cur_tag[0] is not None:
        tag, _cur_tag[0] = _cur_tag[0], None
    if _count is not None:
        _count += 1
    if _prof is None or len(_pool) < 2:
        return fn()
    s, e = _pool.pop(), _pool.pop()
    s.record()
    r = fn()
    e.record()
    if name is None:
        name = lib().dvq_last_kernel().decode() or entry
    if tag is not None:
        name = f"{name} | {tag}"
    _prof.setdefault(name, []).append((s, e, flops, nbytes))
    return r


def _timed_conv(flops, nbytes, entry, call):
    """a conv entry point under _timed: which kernel it lands on is decided -- and reported -- by the library"""
    return _timed(None, flops, nbytes, lambda: check(call(), entry), entry)


def _conv_cost(d: ConvDesc, esize: int):
    """algorithmic cost of one conv pass: 2*M*K*N flops; bytes = input + weights + output once each.  A folded upsample that runs
    as four 2x2 sub-pixel convolutions (conv_subpixel_ok) is still counted with the 9 taps of the function it computes."""
    flops = 2 * d.N * d.OH * d.OW * d.Cout * d.KH * d.KW * d.Cin
    sh, sw = (d.H // 2, d.W // 2) if d.upsample else (d.H, d.W)
    nbytes = esize * (d.N * sh * sw * d.Cin + d.Cout * d.KH * d.KW * d.Cin + d.N * d.OH * d.OW * d.Cout)
    return flops, nbytes


# ---------------------------------------------------------------------------------------------
# VQ
# ---------------------------------------------------------------------------------------------
def vq_prepare(codebook: torch.Tensor) -> torch.Tensor:
    k, d = codebook.shape
    prep = torch.empty(lib().dvq_vq_prep_bytes(k, d), dtype=torch.uint8, device=codebook.device)
    check(lib().dvq_vq_prepare(_p(codebook), k, d, _p(prep), _s()), "dvq_vq_prepare")
    return prep


_vq_ws = {}


def _vq_workspace(n, device):
    """scratch of dvq_vq_argmin: its counters must be zero when a call starts and every call leaves them zero (the re-rank kernel
    re-arms them), so ONE zero-filled buffer per (device, stream, N) serves all calls on that stream -- no zero-fill launch per
    search.  Inside a stream capture a fresh zeroed buffer is used instead (it lives in the capture's pool; the fill is recorded
    with it)."""
    nbytes = lib().dvq_vq_argmin_workspace_bytes(n)
    if torch.cuda.is_current_stream_capturing():
        return torch.zeros(nbytes, dtype=torch.uint8, device=device)
    key = (device.index, torch.cuda.current_stream(device).cuda_stream, n)
    ws = _vq_ws.get(key)
    if ws is None:
        if len(_vq_ws) >= 16:
            _vq_ws.clear()
        ws = _vq_ws[key] = torch.zeros(nbytes, dtype=torch.uint8, device=device)
    return ws


def vq_argmin(x: torch.Tensor, codebook: torch.Tensor, prep: torch.Tensor | None = None, impl: int = 0,
              return_flagged: bool = False):
    """x [N,D] (fp32/bf16), codebook [K,D] fp32 -> idx int64 [N] (exact argmin, lowest index on ties).
    return_flagged: also a device int32 [3] = rows of THIS call settled in fp64 {over all K codes (generic kernel only), over their
    candidate list / flagged residue classes, of those: rows with more candidate classes than an entry lists} -- a COPY made by a
    kernel on this stream (the counters live in scratch shared by every search of this (device, stream, N); under capture in a graph-pool
    buffer each replay refreshes)."""
    n, d = x.shape
    k = codebook.shape[0]
    assert codebook.dtype == torch.float32 and codebook.shape[1] == d
    if prep is None and impl != 1 and d in (64, 128, 256):
        prep = vq_prepare(codebook)
    idx = torch.empty(n, dtype=torch.int64, device=x.device)
    ws = _vq_workspace(n, x.device)
    nbytes = n * d * x.element_size() + k * d * 4 + n * 8
    try:
        _timed("vq_argmin", 2 * n * k * d, nbytes, lambda: check(
            lib().dvq_vq_argmin(_p(x), dt(x), _p(codebook), _p(prep), n, k, d, _p(idx), _p(ws), impl, _s()), "dvq_vq_argmin"))
    except Exception:
        _vq_ws.clear()            # a failed call may leave the counters armed
        raise
    if return_flagged:
        return idx, ws[16:28].view(torch.int32).mul(1)
    return idx


def vq_distances(x, codebook, out=None):
    """x [N,D] (fp32/bf16), codebook [K,D] fp32 -> fp32 [N,K] squared distances (the reference's addmm formula); analysis API"""
    n, d = x.shape
    k = codebook.shape[0]
    if out is None:
        out = torch.empty(n, k, dtype=torch.float32, device=x.device)
    step = 1 << 19
    for a in range(0, n, step):
        b = min(n, a + step)
        check(lib().dvq_vq_distances(_p(x[a:b]), dt(x), _p(codebook), b - a, k, d, _p(out[a:b]), _s()), "dvq_vq_distances")
    return out


def vq_gather_loss(x, codebook, idx, mask=None):
    n, d = x.shape
    xq = torch.empty_like(x)
    loss_sum = torch.zeros(1, dtype=torch.float64, device=x.device)
    check(lib().dvq_vq_gather_loss(_p(x), dt(x), _p(codebook), _p(idx), _p(mask), n, d, _p(xq), _p(loss_sum), _s()),
          "dvq_vq_gather_loss")
    return xq, loss_sum


def vq_backward(g_xq, x, codebook, idx, mask, coef_dev):
    n, d = x.shape
    dx = torch.empty_like(x)
    check(lib().dvq_vq_backward(_p(g_xq), _p(x), dt(x), _p(codebook), _p(idx), _p(mask), _p(coef_dev), n, d, _p(dx), _s()),
          "dvq_vq_backward")
    return dx


def vq_embed(codebook, idx, dtype=torch.float32, out=None):
    d = codebook.shape[1]
    flat = idx.reshape(-1).contiguous()
    if out is None:
        out = torch.empty(flat.numel(), d, dtype=dtype, device=codebook.device)
    check(lib().dvq_vq_embed(_p(codebook), _p(flat), flat.numel(), d, dt(dtype), _p(out), _s()), "dvq_vq_embed")
    return out.reshape(*idx.shape, d)


def vq_ema_stats(x, idx, k, out=None):
    n, d = x.shape
    stats = torch.empty(k, d + 1, dtype=torch.float32, device=x.device) if out is None else out
    check(lib().dvq_vq_ema_stats(_p(x), dt(x), _p(idx), n, k, d, _p(stats), _s()), "dvq_vq_ema_stats")
    return stats


def vq_ema_apply(stats, restart_rows, decay, eps, cluster_size_ema, embed_ema, weight):
    k, d = embed_ema.shape
    check(lib().dvq_vq_ema_apply(_p(stats), _p(restart_rows), decay, eps, k, d, _p(cluster_size_ema), _p(embed_ema),
                                 _p(weight), None, _s()), "dvq_vq_ema_apply")


# -- gradient-trained codebook (csrc/vq_trained.hip) ------------------------------------------------
def vq_trained_prepare(codebook: torch.Tensor, cosine: bool) -> torch.Tensor:
    """split planes + per-code bias of dvq_vq_sample_argmax (cosine: rows normalised); rebuild when the codebook changes"""
    k, d = codebook.shape
    assert codebook.dtype == torch.float32
    prep = torch.empty(lib().dvq_vq_trained_prep_bytes(k, d), dtype=torch.uint8, device=codebook.device)
    check(lib().dvq_vq_trained_prepare(_p(codebook), k, d, int(bool(cosine)), _p(prep), _s()), "dvq_vq_trained_prepare")
    return prep


def vq_sample_argmax(x, prep, k, cosine: bool, temp: float = 0.0, state=None, codebook=None):
    """x [N,D] (fp32/bf16), prep = vq_trained_prepare(codebook [k,D], cosine) -> idx int64 [N] = argmax_k (score / temp + Gumbel noise),
    lowest index on ties; temp == 0: no noise.  state: device int64 [2] {seed, counter}; the counter advances by one per noisy call.
    codebook: the raw fp32 [k,D] rows, needed by the noiseless cosine search (its near ties are re-ranked in fp64: exact)."""
    n, d = x.shape
    idx = torch.empty(n, dtype=torch.int64, device=x.device)
    nbytes = n * d * x.element_size() + k * d * 4 + n * 8
    _timed("vq_sample_argmax", 2 * n * k * d, nbytes, lambda: check(
        lib().dvq_vq_sample_argmax(_p(x), dt(x), _p(prep), _p(codebook), n, k, d, int(bool(cosine)), float(temp), _p(state), _p(idx), _s()),
        "dvq_vq_sample_argmax"))
    return idx


def vq_gumbel_noise(seed: int, counter: int, n: int, k: int, device) -> torch.Tensor:
    """fp32 [n,k]: the noise vq_sample_argmax adds while its state holds (seed, counter); tests and analysis"""
    out = torch.empty(n, k, dtype=torch.float32, device=device)
    check(lib().dvq_vq_gumbel_noise(int(seed) & (2 ** 64 - 1), int(counter) & (2 ** 64 - 1), n, k, _p(out), _s()), "dvq_vq_gumbel_noise")
    return out


def vq_codebook_grad(x, codebook, idx, mask, coef_dev, grad):
    """grad [K,D] fp32 += coef_dev[0] * sum_{n: idx[n] = k} mask[n] (codebook[k] - x[n]); bit-reproducible under set_deterministic"""
    n, d = x.shape
    k = codebook.shape[0]
    assert grad.dtype == torch.float32 and tuple(grad.shape) == (k, d) and codebook.dtype == torch.float32
    _timed("vq_codebook_grad", 2 * n * d, n * d * x.element_size() + n * 8 + 2 * k * d * 4, lambda: check(
        lib().dvq_vq_codebook_grad(_p(x), dt(x), _p(codebook), _p(idx), _p(mask), _p(coef_dev), n, k, d, _p(grad), _s()),
        "dvq_vq_codebook_grad"))
    return grad


def vq_mask_ratio(mask):
    """fp32 device scalar [1] = numel / sum(mask)"""
    out = torch.empty(1, dtype=torch.float32, device=mask.device)
    check(lib().dvq_vq_mask_ratio(_p(mask), mask.numel(), _p(out), _s()), "dvq_vq_mask_ratio")
    return out


def vq_rownorm(e):
    """e [K,D] fp32 -> (w = e / max(|e|, 1e-12) per row, inv [K] = the reciprocals)"""
    k, d = e.shape
    w = torch.empty_like(e)
    inv = torch.empty(k, dtype=torch.float32, device=e.device)
    check(lib().dvq_vq_rownorm(_p(e), k, d, _p(w), _p(inv), _s()), "dvq_vq_rownorm")
    return w, inv


def vq_ortho_sumsq(g, k, scale):
    """g [k,k] fp32 -= I in place -> fp32 device scalar [1] = scale * sum(g^2) (fixed summation order)"""
    scratch = torch.empty(lib().dvq_vq_ortho_scratch_bytes(), dtype=torch.uint8, device=g.device)
    out = torch.empty(1, dtype=torch.float32, device=g.device)
    check(lib().dvq_vq_ortho_sumsq(_p(g), k, float(scale), _p(scratch), _p(out), _s()), "dvq_vq_ortho_sumsq")
    return out


def vq_rownorm_bwd(w, inv, dw, coef_dev, scale, grad):
    """grad [K,D] += coef_dev[0] * scale * inv[k] * (dw[k] - w[k] (w[k] . dw[k]))"""
    k, d = w.shape
    check(lib().dvq_vq_rownorm_bwd(_p(w), _p(inv), _p(dw), _p(coef_dev), float(scale), k, d, _p(grad), _s()), "dvq_vq_rownorm_bwd")
    return grad


# ---------------------------------------------------------------------------------------------
# entropy / gate
# ---------------------------------------------------------------------------------------------
def patch_entropy_gate(img: torch.Tensor, patch: int, threshold: float | None, bins=(-1.0, 1.0)):
    """img NCHW fp32 [B,3,H,W] -> (entropy [B,h,w] fp32, gate int64 [B,h,w,2] or None); bins = range of the 32 histogram bins"""
    b, c, h, w = img.shape
    assert c == 3 and img.dtype == torch.float32
    ent = torch.empty(b, h // patch, w // patch, dtype=torch.float32, device=img.device)
    gate = None
    if threshold is not None:
        gate = torch.empty(b, h // patch, w // patch, 2, dtype=torch.int64, device=img.device)
    if tuple(bins) == (-1.0, 1.0):
        check(lib().dvq_patch_entropy_gate(_p(img), b, h, w, patch, float(threshold or 0.0), _p(ent), _p(gate), _s()),
              "dvq_patch_entropy_gate")
    else:
        check(lib().dvq_patch_entropy_gate_range(_p(img), b, h, w, patch, float(bins[0]), float(bins[1]), float(threshold or 0.0),
                                                 _p(ent), _p(gate), _s()), "dvq_patch_entropy_gate_range")
    return ent, gate


# ---------------------------------------------------------------------------------------------
# GroupNorm (+swish)
# ---------------------------------------------------------------------------------------------
def gn_stats(x, groups=32):
    """x NHWC -> fp64 [N,G,2] (sum, sum of squares)"""
    n, c = x.shape[0], x.shape[-1]
    hw = x.numel() // (n * c)
    stats = zeros_small((n, groups, 2), torch.float64, x.device)
    check(lib().dvq_gn_stats(_p(x), dt(x), n, hw, c, groups, _p(stats), _s()), "dvq_gn_stats")
    return stats


def gn_forward(x, gamma, beta, groups=32, eps=1e-6, silu=True, stats=None):
    """x NHWC [N,H,W,C]; returns (y, mean_rstd [N,G,2] fp32).  `stats` may come from a producer's fused epilogue."""
    n, c = x.shape[0], x.shape[-1]
    hw = x.numel() // (n * c)
    if stats is None:
        stats = gn_stats(x, groups)
    y = torch.empty_like(x)
    mr = torch.empty(n, groups, 2, dtype=torch.float32, device=x.device)
    check(lib().dvq_gn_apply(_p(x), dt(x), n, hw, c, groups, eps, _p(stats), _p(gamma), _p(beta), int(silu), _p(y), _p(mr),
                             _s()), "dvq_gn_apply")
    return y, mr


def gn_scale_shift(x, gamma, beta, groups=32, eps=1e-6, stats=None):
    """per-(n,c) {scale, shift} fp32 [N,C,2] for the fused conv prologue + mean_rstd [N,G,2] for the backward"""
    n, c = x.shape[0], x.shape[-1]
    hw = x.numel() // (n * c)
    if stats is None:
        stats = gn_stats(x, groups)
    ss = torch.empty(n, c, 2, dtype=torch.float32, device=x.device)
    mr = torch.empty(n, groups, 2, dtype=torch.float32, device=x.device)
    check(lib().dvq_gn_scale_shift(_p(stats), _p(gamma), _p(beta), n, hw, c, groups, eps, _p(ss), _p(mr), _s()),
          "dvq_gn_scale_shift")
    return ss, mr


def gn_backward(x, dy, mean_rstd, gamma, beta, dgamma, dbeta, groups=32, silu=True, addend=None, fixed_stats=False):
    """dgamma/dbeta (fp32 [C]) are accumulated into; returns dx.  fixed_stats: mean / rstd are constants, not functions of x (ActNorm:
    a per-channel affine): the statistic terms of dx are dropped by zeroing the reduced sums, dx = rstd * gamma * dz"""
    n, c = x.shape[0], x.shape[-1]
    hw = x.numel() // (n * c)
    red = zeros_small((n, groups, 2), torch.float64, x.device)
    # per-block partials + fold kernel instead of thousands of atomics per address
    part = torch.empty(lib().dvq_gn_bwd_partial_bytes(n, hw, c), dtype=torch.uint8, device=x.device)
    check(lib().dvq_gn_bwd_reduce(_p(x), _p(dy), dt(x), n, hw, c, groups, _p(mean_rstd), _p(gamma), _p(beta), int(silu),
                                  _p(red), _p(dgamma), _p(dbeta), _p(part), _s()), "dvq_gn_bwd_reduce")
    if fixed_stats:
        red.zero_()
    dx = torch.empty_like(x)
    check(lib().dvq_gn_bwd_dx(_p(x), _p(dy), dt(x), n, hw, c, groups, _p(mean_rstd), _p(gamma), _p(beta), int(silu),
                              _p(red), _p(addend), _p(dx), _s()), "dvq_gn_bwd_dx")
    return dx


# ---------------------------------------------------------------------------------------------
# convolution
# ---------------------------------------------------------------------------------------------
def conv_desc(n, h, w, cin, cout, kh, kw, stride, pad_t, pad_l, oh, ow, upsample, dtype, impl=0) -> ConvDesc:
    return ConvDesc(n, h, w, cin, oh, ow, cout, kh, kw, stride, pad_t, pad_l, int(upsample), dt(dtype), impl)


PACK_OHWI, PACK_SUBPIXEL = 256, 512      # bits 8 / 9 of dvq_pack_weight's dtype (include/dvq_hip.h)


def subpixel_pack_views(wbuf, wtbuf, cout, cin):
    """flat pack buffers of a sub-pixel-eligible 3x3 conv -> (w [Cout,3,3,Cin], wt [Cin,3,3,Cout], Weff [4,Cout,4,Cin],
    WeffT [Cin,4,4,Cout]): the sub-pixel packs sit behind the 3x3 packs, the layout dvq_conv2d_fwd / _dgrad read with upsample == 2"""
    n9 = cout * 9 * cin
    return (wbuf[:n9].view(cout, 3, 3, cin), wtbuf[:n9].view(cin, 3, 3, cout), wbuf[n9:].view(4, cout, 4, cin),
            wtbuf[n9:].view(cin, 4, 4, cout))


def pack_weight(master_oihw, cin_p, cout_p, dtype, want_w=True, want_wt=True, subpixel=False):
    """subpixel: flat (w | Weff) and (wt | WeffT) buffers, see subpixel_pack_views"""
    cout, cin, kh, kw = master_oihw.shape
    dev = master_oihw.device
    if subpixel:
        w = torch.empty(25 * cout * cin, dtype=dtype, device=dev)
        wt = torch.empty(25 * cout * cin, dtype=dtype, device=dev)
        check(lib().dvq_pack_weight(_p(master_oihw), cout, cin, kh, kw, cin_p, cout_p, dt(dtype) | PACK_SUBPIXEL, _p(w), _p(wt), _s()),
              "dvq_pack_weight")
        return w, wt
    w = torch.empty(cout, kh, kw, cin_p, dtype=dtype, device=dev) if want_w else None
    wt = torch.zeros(cin_p, kh, kw, cout_p, dtype=dtype, device=dev) if want_wt else None   # rows >= Cin stay zero
    check(lib().dvq_pack_weight(_p(master_oihw), cout, cin, kh, kw, cin_p, cout_p, dt(dtype), _p(w), _p(wt), _s()),
          "dvq_pack_weight")
    return w, wt


def pack_weight_into(master, cin_p, cout_p, dtype, w, wt, subpixel=False):
    cout, cin, kh, kw = master.shape
    flag = dt(dtype) | (PACK_OHWI if is_ohwi(master) else 0) | (PACK_SUBPIXEL if subpixel else 0)
    check(lib().dvq_pack_weight(_praw(master), cout, cin, kh, kw, cin_p, cout_p, flag, _p(w), _p(wt), _s()),
          "dvq_pack_weight")


def unpack_wgrad(dw, grad_oihw, cin_p):
    cout, cin, kh, kw = grad_oihw.shape
    check(lib().dvq_unpack_wgrad(_p(dw), cout, cin, kh, kw, cin_p, _p(grad_oihw), _s()), "dvq_unpack_wgrad")


def conv_fused_ok(d: ConvDesc) -> bool:
    return bool(lib().dvq_conv3x3_fused_ok(C.byref(d)))


def conv_subpixel_ok(d: ConvDesc) -> bool:
    """a folded nearest-x2 upsample + 3x3 that the library runs as four 2x2 sub-pixel convolutions when handed the sub-pixel packs"""
    return bool(lib().dvq_conv3x3_subpixel_ok(C.byref(d)))


def _with_subpixel(d: ConvDesc) -> ConvDesc:
    """the descriptor with upsample = 2: the weight argument carries the sub-pixel pack behind its 3x3 pack"""
    d2 = ConvDesc.from_buffer_copy(d)
    d2.upsample = 2
    return d2


ACT_NONE, ACT_SWISH, ACT_LRELU, ACT_RELU = 0, 1, 2, 3      # include/dvq_hip.h DVQ_ACT_*


PASS_FWD, PASS_DGRAD, PASS_WGRAD = 0, 1, 2      # include/dvq_hip.h DVQ_PASS_*


def conv_scratch_bytes(d: ConvDesc, pass_: int) -> int:
    """bytes of scratch with which the library runs this pass as a launch-level fp32x3 scheme (bf16 planes of the fp32 operands on the
    bf16 kernels); 0: it has no such route for this descriptor in the current compute mode"""
    return int(lib().dvq_conv2d_scratch_bytes(C.byref(d), pass_))


def _x3_scratch(d: ConvDesc, pass_: int, on: bool, device):
    """(scratch from the caching allocator or None, its size).  `on` False (A/B switches DVQ_X3_HALO=0, DVQ_X3_WGRAD_PLANES=0): no
    scratch is passed and the pass stays on the fp32 kernel that splits at every fragment read"""
    need = conv_scratch_bytes(d, pass_) if on else 0
    return (torch.empty(need, dtype=torch.uint8, device=device) if need else None), need


def conv2d_fwd(d: ConvDesc, x, w, bias, residual=None, gn_ss=None, out_stats=None, out_groups=0, act=ACT_NONE, subpixel=False):
    """subpixel: `w` is followed by the sub-pixel pack (subpixel_pack_views) and d is accepted by conv_subpixel_ok"""
    y = torch.empty(d.N, d.OH, d.OW, d.Cout, dtype=x.dtype, device=x.device)
    fl, nb = _conv_cost(d, x.element_size())
    scratch, need = _x3_scratch(d, PASS_FWD, rt.switch("DVQ_X3_HALO") != "0", x.device)
    if _shape_tags():     # per-shape tables split the forward by epilogue / prologue variant (tools/debug/step_shapes.py)
        _tag(d, ("fwd x3 halo" if need else "fwd") + ("+res" if residual is not None else "") + ("+gn" if gn_ss is not None else "") +
             ("+st" if out_stats is not None else "") + ("+act" if act != ACT_NONE else ""))
    if out_stats is not None:
        ensure_workspace(x.device)        # per-tile statistics partials of the halo kernel
    dc = _with_subpixel(d) if subpixel else d
    _timed_conv(fl, nb, "dvq_conv2d_fwd", lambda:
        lib().dvq_conv2d_fwd(C.byref(dc), _p(x), _p(w), _p(bias), _p(residual), _p(y), _p(gn_ss), _p(out_stats), out_groups, act,
                             _p(scratch), need, _s()))
    return y


def conv2d_dgrad(d: ConvDesc, dy, wt, mask=None, mask_act=ACT_NONE, subpixel=False):
    """mask: output of the activation that produced this conv's input; the gradient is gated through it.
    subpixel: `wt` is followed by the sub-pixel pack and d is accepted by conv_subpixel_ok -- the gradient of a folded upsample is
    then formed at the stored resolution, without the full-resolution workspace"""
    sh, sw = (d.H // 2, d.W // 2) if d.upsample else (d.H, d.W)
    dx = torch.empty(d.N, sh, sw, d.Cin, dtype=dy.dtype, device=dy.device)
    ws = torch.empty(d.N, d.H, d.W, d.Cin, dtype=dy.dtype, device=dy.device) if d.upsample and not subpixel else None
    fl, nb = _conv_cost(d, dy.element_size())
    scratch, need = _x3_scratch(d, PASS_DGRAD, rt.switch("DVQ_X3_HALO") != "0", dy.device)
    _tag(d, "dgrad x3 halo" if need else "dgrad")
    dc = _with_subpixel(d) if subpixel else d
    _timed_conv(fl, nb, "dvq_conv2d_dgrad", lambda:
        lib().dvq_conv2d_dgrad(C.byref(dc), _p(dy), _p(wt), _p(dx), _p(ws), _p(mask), mask_act, _p(scratch), need, _s()))
    return dx


_workspace = {}
# 8 per-stream slots (csrc/misc.hip: dvq_workspace_stream) of 80 MB: 256 workgroups x (9 x 128 x 64 + 128) fp32 partials of the
# split-K weight-gradient kernels
WORKSPACE_BYTES = 8 * (80 << 20)


def workspace_release(stream):
    """give back the scratch slot a (capture) stream holds -- called when its recording is dropped"""
    if _workspace:
        lib().dvq_workspace_release(C.c_void_p(int(stream.cuda_stream)))


def copy_kernel_(dst, src):
    """dst <- src through an elementwise KERNEL.  torch's copy_ between contiguous same-dtype tensors is a hipMemcpyAsync, which a
    recorded step keeps as a 1-D memcpy node -- the one node kind a launch list (csrc/cmdlist.hip) cannot re-issue.  x * 1 is exact."""
    return torch.mul(src, 1, out=dst)


class CmdList:
    """launch list of one captured segment (csrc/cmdlist.hip); `graph` is the torch.cuda.CUDAGraph(keep_graph=True) whose nodes
    own the argument blocks -- kept alive here, released after the list"""

    def __init__(self, graph):
        self.graph = graph
        h = C.c_void_p()
        check(lib().dvq_cmdlist_create(C.c_void_p(int(graph.raw_cuda_graph())), C.byref(h)), "dvq_cmdlist_create")
        self.handle = h
        info = (C.c_int64 * 4)()
        check(lib().dvq_cmdlist_info(h, info), "dvq_cmdlist_info")
        self.kernels, self.side_kernels, self.waits = int(info[0]), int(info[1]), int(info[2])
        self.other, self.side_open = int(info[3]) & 0xffffffff, bool(int(info[3]) >> 32)

    def replay(self, main, side):
        check(lib().dvq_cmdlist_replay(self.handle, C.c_void_p(int(main.cuda_stream)), C.c_void_p(int(side.cuda_stream))),
              "dvq_cmdlist_replay")

    def __del__(self):
        try:
            if self.handle:
                lib().dvq_cmdlist_destroy(self.handle)
                self.handle = None
        except Exception:
            pass
        self.graph = None


def ensure_workspace(device):
    """register the process-wide scratch buffer of libdvq_hip (kept alive here)"""
    device = torch.device(device)
    if _workspace.get("dev") != device:
        buf = torch.empty(WORKSPACE_BYTES, dtype=torch.uint8, device=device)
        check(lib().dvq_set_workspace(buf.data_ptr(), buf.numel()), "dvq_set_workspace")
        _workspace.update(dev=device, buf=buf)


def split_bf16_planes(x2d, cout=None):
    """fp32 [rows, C] -> (hi, lo) bf16 [rows, cout]: hi = RNE(x), lo = RNE(x - hi); channels >= C are zero"""
    rows, c = x2d.shape
    cout = c if cout is None else cout
    hi = torch.empty(rows, cout, dtype=torch.bfloat16, device=x2d.device)
    lo = torch.empty_like(hi)
    check(lib().dvq_split_bf16_planes(_p(x2d), _p(hi), _p(lo), rows, c, cout, _s()), "dvq_split_bf16_planes")
    return hi, lo


def conv2d_wgrad_oihw(d: ConvDesc, x, dy, cin_real, cout_real, grad_oihw, db=None, gn_ss=None):
    """accumulate the weight gradient straight into the [Cout,Cin,KH,KW] fp32 grad (and db into [Cout]);
    gn_ss: the fused GroupNorm+swish of the forward is re-applied to x inside the kernel"""
    fl, nb = _conv_cost(d, x.element_size())
    ensure_workspace(x.device)
    scratch, need = _x3_scratch(d, PASS_WGRAD, rt.switch("DVQ_X3_WGRAD_PLANES") != "0", x.device)
    _tag(d, "wgrad x3 planes" if need else "wgrad")
    _timed_conv(fl, nb, "dvq_conv2d_wgrad", lambda:
        lib().dvq_conv2d_wgrad(C.byref(d), _p(x), _p(dy), cin_real, cout_real, _praw(grad_oihw), _p(db),
                               int(is_ohwi(grad_oihw)), _p(gn_ss), _p(scratch), need, _s()))


def set_deterministic(on: bool):
    """opt-in: every floating-point reduction of a training step runs in a fixed order -- per-split partials + a fold, or one owner per
    output element -- never through float atomics with several writers (bit-reproducible steps; docs/design/21-reproducible-training.md)"""
    check(lib().dvq_set_deterministic(int(bool(on))), "dvq_set_deterministic")
    _det[0] = bool(on)


def deterministic() -> bool:
    _det[0] = bool(lib().dvq_deterministic())
    return _det[0]


def unordered_launches() -> int:
    """process-wide count of launches whose floating-point result depends on arrival order (float atomics with several writers per
    address); it does not move across calls made in deterministic mode"""
    return int(lib().dvq_unordered_launches())


def pack_weights_multi(table_dev, n_entries, total_work):
    check(lib().dvq_pack_weights_multi(_p(table_dev), n_entries, total_work, _s()), "dvq_pack_weights_multi")


def linear_pack_multi(table_dev, n_entries, total_tiles):
    check(lib().dvq_linear_pack_multi(_p(table_dev), n_entries, total_tiles, _s()), "dvq_linear_pack_multi")


# ---------------------------------------------------------------------------------------------
# zero arena: one memset per step instead of one torch.zeros per small statistics buffer
# ---------------------------------------------------------------------------------------------
_arena = {"buf": None, "off": 0}


def arena_reset(device=None, nbytes=8 << 20):
    a = _arena
    if a["buf"] is None or (device is not None and a["buf"].device != torch.device(device)):
        a["buf"] = torch.zeros(nbytes, dtype=torch.uint8, device=device or "cuda")
    else:
        a["buf"].zero_()
    a["off"] = 0


def zeros_small(shape, dtype, device):
    """zero-initialised small buffer: a slice of the per-step arena when one is active, else torch.zeros"""
    a = _arena
    n = 1
    for s_ in shape:
        n *= int(s_)
    nb = (n * torch.empty((), dtype=dtype).element_size() + 255) // 256 * 256
    if a["buf"] is None or a["buf"].device != torch.device(device) or a["off"] + nb > a["buf"].numel():
        return torch.zeros(shape, dtype=dtype, device=device)
    out = a["buf"][a["off"]:a["off"] + nb].view(dtype)[:n].view(shape)
    a["off"] += nb
    return out


def nchw_to_nhwc_pad(img, cp, dtype):
    b, c, h, w = img.shape
    out = torch.empty(b, h, w, cp, dtype=dtype, device=img.device)
    check(lib().dvq_nchw_to_nhwc_pad(_p(img), b, c, h, w, cp, dt(dtype), _p(out), _s()), "dvq_nchw_to_nhwc_pad")
    return out


def nhwc_pad_to_nchw(x, c):
    b, h, w, cp = x.shape
    out = torch.empty(b, c, h, w, dtype=torch.float32, device=x.device)
    check(lib().dvq_nhwc_pad_to_nchw(_p(x), dt(x), b, c, h, w, cp, _p(out), _s()), "dvq_nhwc_pad_to_nchw")
    return out


# ---------------------------------------------------------------------------------------------
# GEMMs / attention pieces
# ---------------------------------------------------------------------------------------------
def probe_mfma_rate(random_operands=True):
    """(TFLOP/s, shader MHz) a register-only bf16 MFMA loop sustains on the current device (diagnostics for bench.py)"""
    tf, mhz = C.c_float(0.0), C.c_float(0.0)
    check(lib().dvq_probe_mfma_rate(int(bool(random_operands)), C.byref(tf), C.byref(mhz), _s()), "dvq_probe_mfma_rate")
    return float(tf.value), float(mhz.value)


def gemm_nt(a, b, m, n, k, lda, ldb, ldc, batch=1, sa=0, sb=0, sc=0, alpha=1.0, bias=None, bias_mode=0, out=None,
            impl=0):
    """C[b][m][n] = alpha * sum_k A[b][m][k] B[b][n][k] (+bias).  a, b, out are flat device tensors.  impl: _lib.IMPL_*"""
    if out is None:
        out = torch.empty(batch * m * ldc if sc == 0 else batch * sc, dtype=a.dtype, device=a.device)
    es = a.element_size()
    _timed("gemm_nt", 2 * batch * m * n * k, es * batch * (m * k + n * k + m * n), lambda: check(
        lib().dvq_gemm_nt(_p(a), _p(b), _p(out), dt(a), m, n, k, lda, ldb, ldc, batch, sa, sb, sc, alpha, _p(bias),
                          bias_mode, impl, _s()), "dvq_gemm_nt"))
    return out


def gemm_tn(a, b, mred, i, j, lda, ldb, ldc, batch=1, sa=0, sb=0, sc=0, out=None, impl=0, colsum=None):
    """C[b][i][j] (fp32) += sum_m A[b][m][i] B[b][m][j]; colsum (fp32 [i], batch 1): += column sums of A from the same pass"""
    if out is None:
        out = torch.zeros(batch * (sc if sc else i * ldc), dtype=torch.float32, device=a.device)
    es = a.element_size()
    if a.is_cuda and es == 2 and mred >= 1024 and i >= 256 and j >= 256:
        ensure_workspace(a.device)        # split partials of the 256 x 256 kernel (fold kernel instead of fp32 atomics)
    _timed("gemm_tn", 2 * batch * mred * i * j, es * batch * mred * (i + j) + 4 * batch * i * j, lambda: check(
        lib().dvq_gemm_tn(_p(a), _p(b), _p(out), _p(colsum), dt(a), mred, i, j, lda, ldb, ldc, batch, sa, sb, sc, impl, _s()),
        "dvq_gemm_tn"))
    return out


def softmax_rows(s, rows, length, scale):
    p = torch.empty_like(s)
    check(lib().dvq_softmax_rows(_p(s), dt(s), rows, length, scale, _p(p), _s()), "dvq_softmax_rows")
    return p


def softmax_rows_bwd(p, dp, rows, length, scale):
    ds = torch.empty_like(p)
    check(lib().dvq_softmax_rows_bwd(_p(p), _p(dp), dt(p), rows, length, scale, _p(ds), _s()), "dvq_softmax_rows_bwd")
    return ds


def transpose(x, batch, r, c):
    out = torch.empty_like(x)
    check(lib().dvq_transpose(_p(x), dt(x), batch, r, c, _p(out), _s()), "dvq_transpose")
    return out


# ---------------------------------------------------------------------------------------------
# small ops
# ---------------------------------------------------------------------------------------------
def dual_merge(h_fine, h_coarse, grain):
    b, h, w, c = h_coarse.shape
    out = torch.empty_like(h_fine)
    mask = torch.empty(b, 2 * h, 2 * w, dtype=torch.float32, device=h_fine.device)
    check(lib().dvq_dual_merge(_p(h_fine), _p(h_coarse), _p(grain), dt(h_fine), b, h, w, c, _p(out), _p(mask), _s()),
          "dvq_dual_merge")
    return out, mask


def dual_merge_bwd(g_dual, grain):
    b, h2, w2, c = g_dual.shape
    h, w = h2 // 2, w2 // 2
    gf = torch.empty_like(g_dual)
    gc = torch.empty(b, h, w, c, dtype=g_dual.dtype, device=g_dual.device)
    check(lib().dvq_dual_merge_bwd(_p(g_dual), _p(grain), dt(g_dual), b, h, w, c, _p(gf), _p(gc), _s()),
          "dvq_dual_merge_bwd")
    return gf, gc


def add(a, b):
    y = torch.empty_like(a)
    check(lib().dvq_add(_p(a), _p(b), dt(a), a.numel(), _p(y), _s()), "dvq_add")
    return y


def channel_shift_add8(a, b, shift):
    """a, b: [..., 8] bf16 pixels -> a + (b moved up by `shift` channels)"""
    assert a.shape == b.shape and a.shape[-1] == 8 and a.dtype == torch.bfloat16
    y = torch.empty_like(a)
    check(lib().dvq_channel_shift_add8(_p(a), _p(b), dt(a), a.numel() // 8, int(shift), _p(y), _s()), "dvq_channel_shift_add8")
    return y


def add_bias_bcast(x, bias):
    batch = x.shape[0]
    y = torch.empty_like(x)
    check(lib().dvq_add_bias_bcast(_p(x), _p(bias), dt(x), batch, x.numel() // batch, _p(y), _s()), "dvq_add_bias_bcast")
    return y


def sum_batch(x, out):
    batch = x.shape[0]
    check(lib().dvq_sum_batch(_p(x), dt(x), batch, x.numel() // batch, _p(out), _s()), "dvq_sum_batch")
    return out


def cast(x, dtype):
    if x.dtype == dtype:
        return x
    out = torch.empty(x.shape, dtype=dtype, device=x.device)
    check(lib().dvq_cast(_p(x), dt(x), _p(out), dt(dtype), x.numel(), _s()), "dvq_cast")
    return out


def l1_loss(x, xrec, scale_dev=None, want_grad=False):
    loss_sum = torch.zeros(1, dtype=torch.float64, device=x.device)
    g = torch.empty_like(xrec) if want_grad else None
    check(lib().dvq_l1_loss(_p(x), _p(xrec), x.numel(), _p(loss_sum), _p(scale_dev), _p(g), _s()), "dvq_l1_loss")
    return loss_sum, g


def adam_step(p, g, m, v, lr, beta1, beta2, eps, step):
    check(lib().dvq_adam(_p(p), _p(g), _p(m), _p(v), p.numel(), lr, beta1, beta2, eps, step, _s()), "dvq_adam")


def fill(p, value):
    check(lib().dvq_fill_f32(_p(p), float(value), p.numel(), _s()), "dvq_fill_f32")


# ---------------------------------------------------------------------------------------------
# loss networks (LPIPS / PatchGAN)
# ---------------------------------------------------------------------------------------------
def affine_channels(x, a, b=None):
    """y[..., c] = x[..., c] * a[c] + b[c]"""
    y = torch.empty_like(x)
    check(lib().dvq_affine_channels(_p(x), dt(x), x.numel(), x.shape[-1], _p(a), _p(b), _p(y), _s()), "dvq_affine_channels")
    return y


def axpy_dev(a, b, scale_dev):
    """a + scale_dev[0] * b (scale_dev: fp32 device scalar)"""
    y = torch.empty_like(a)
    check(lib().dvq_axpy_dev(_p(a), _p(b), _p(scale_dev), dt(a), a.numel(), _p(y), _s()), "dvq_axpy_dev")
    return y


def maxpool2x2(x):
    n, h2, w2, c = x.shape
    y = torch.empty(n, h2 // 2, w2 // 2, c, dtype=x.dtype, device=x.device)
    check(lib().dvq_maxpool2x2(_p(x), dt(x), n, h2 // 2, w2 // 2, c, _p(y), _s()), "dvq_maxpool2x2")
    return y


def maxpool2x2_relu_bwd(a, dpool=None, dtap=None):
    n, h2, w2, c = a.shape
    dz = torch.empty_like(a)
    check(lib().dvq_maxpool2x2_relu_bwd(_p(a), _p(dpool), _p(dtap), dt(a), n, h2 // 2, w2 // 2, c, _p(dz), _s()),
          "dvq_maxpool2x2_relu_bwd")
    return dz


def lpips_head(f0, f1, lin, val, gscale=0.0, want_grad=False, p_drop=0.0, seed=0):
    """val[n] (fp32, accumulated) += LPIPS term of one tap; returns d val / d f1 * gscale (or None).  p_drop > 0: NetLinLayer's
    dropout on the squared differences (hash-seeded mask, the same in the value and in the gradient)"""
    n, c = f0.shape[0], f0.shape[-1]
    hw = f0.numel() // (n * c)
    df1 = torch.empty_like(f1) if want_grad else None
    check(lib().dvq_lpips_head_drop(_p(f0), _p(f1), _p(lin), dt(f0), n, hw, c, _p(val), float(gscale), _p(df1), float(p_drop), int(seed),
                                    _s()), "dvq_lpips_head_drop")
    return df1


# ---------------------------------------------------------------------------------------------
# feature-routed (Gumbel) dual / triple grain pieces
# ---------------------------------------------------------------------------------------------
def avgpool_slice(x, k, out, coff):
    """mean over k x k windows of x [N,h*k,w*k,C] -> channel slice [coff, coff+C) of out [N,h,w,ldy]"""
    n, hk, wk, c = x.shape
    check(lib().dvq_avgpool_slice(_p(x), dt(x), n, hk // k, wk // k, c, k, _p(out), out.shape[-1], coff, _s()), "dvq_avgpool_slice")


def avgpool_slice_bwd(dy, coff, c, k):
    n, h, w, ldy = dy.shape
    dx = torch.empty(n, h * k, w * k, c, dtype=dy.dtype, device=dy.device)
    check(lib().dvq_avgpool_slice_bwd(_p(dy), dt(dy), ldy, coff, n, h, w, c, k, _p(dx), _s()), "dvq_avgpool_slice_bwd")
    return dx


def silu(x):
    y = torch.empty_like(x)
    check(lib().dvq_silu(_p(x), dt(x), x.numel(), _p(y), _s()), "dvq_silu")
    return y


def silu_bwd(x, dy):
    dx = torch.empty_like(x)
    check(lib().dvq_silu_bwd(_p(x), _p(dy), dt(x), x.numel(), _p(dx), _s()), "dvq_silu_bwd")
    return dx


def relu(x):
    y = torch.empty_like(x)
    check(lib().dvq_relu(_p(x), dt(x), x.numel(), _p(y), _s()), "dvq_relu")
    return y


def relu_bwd(x, dy):
    dx = torch.empty_like(x)
    check(lib().dvq_relu_bwd(_p(x), _p(dy), dt(x), x.numel(), _p(dx), _s()), "dvq_relu_bwd")
    return dx


def upsample_nearest2x(x):
    """NHWC [N,h,w,C] -> [N,2h,2w,C] (F.interpolate(scale_factor=2, mode="nearest"))"""
    n, h, w, c = x.shape
    y = torch.empty(n, 2 * h, 2 * w, c, dtype=x.dtype, device=x.device)
    check(lib().dvq_upsample_nearest2x(_p(x), dt(x), n, h, w, c, _p(y), _s()), "dvq_upsample_nearest2x")
    return y


def upsample_nearest2x_bwd(dy):
    n, h2, w2, c = dy.shape
    dx = torch.empty(n, h2 // 2, w2 // 2, c, dtype=dy.dtype, device=dy.device)
    check(lib().dvq_upsample_nearest2x_bwd(_p(dy), dt(dy), n, h2 // 2, w2 // 2, c, _p(dx), _s()), "dvq_upsample_nearest2x_bwd")
    return dx


def _ptr_array(tensors):
    arr = (C.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])
    for t in tensors:
        _p(t)                 # device / contiguity checks
    return arr


def grain_merge(heads, idx, scale=None):
    """heads: [coarsest, ..., finest] NHWC; idx int64 [N,hc,wc]; scale fp32 [N,hc,wc] or None -> (merged, codebook mask)"""
    n, hc, wc, c = heads[0].shape
    f = 1 << (len(heads) - 1)
    out = torch.empty(n, hc * f, wc * f, c, dtype=heads[0].dtype, device=heads[0].device)
    mask = torch.empty(n, hc * f, wc * f, dtype=torch.float32, device=out.device)
    arr = _ptr_array(heads)
    check(lib().dvq_grain_merge(arr, len(heads), _p(idx), _p(scale), dt(out), n, hc, wc, c, _p(out), _p(mask), _s()),
          "dvq_grain_merge")
    return out, mask


def grain_merge_bwd(g_out, heads, idx, scale=None, want_dscale=False):
    """-> ([d head_l], d scale or None)"""
    n, hc, wc, c = heads[0].shape
    dheads = [torch.empty_like(h) for h in heads]
    dscale = torch.empty(n, hc, wc, dtype=torch.float32, device=g_out.device) if want_dscale else None
    check(lib().dvq_grain_merge_bwd(_p(g_out), _ptr_array(heads), len(heads), _p(idx), _p(scale), dt(g_out), n, hc, wc, c,
                                    _ptr_array(dheads), _p(dscale), _s()), "dvq_grain_merge_bwd")
    return dheads, dscale


# ---------------------------------------------------------------------------------------------
# StackGPT building blocks
# ---------------------------------------------------------------------------------------------
def layernorm_fwd(x2d, gamma, beta, eps=1e-5, want_stats=True):
    rows, c = x2d.shape
    y = torch.empty_like(x2d)
    mr = torch.empty(rows, 2, dtype=torch.float32, device=x2d.device) if want_stats else None
    check(lib().dvq_layernorm_fwd(_p(x2d), dt(x2d), rows, c, eps, _p(gamma), _p(beta), _p(y), _p(mr), _s()), "dvq_layernorm_fwd")
    return y, mr


def layernorm_bwd(x2d, dy, mr, gamma, dgamma, dbeta, dres=None, drop=None):
    """dx (+ dres: the gradient of the residual stream that by-passes the normalisation, added in the same pass).
    drop = (p, seed): also returns dropout(dx, p, seed) -- the same decisions as `dropout(dx, p, seed)` -- as a second tensor"""
    rows, c = x2d.shape
    dx = torch.empty_like(x2d)
    ensure_workspace(x2d.device)          # per-workgroup dgamma / dbeta partials + fold kernel instead of a million atomics
    if drop is not None and drop[0] > 0.0:
        dxd = torch.empty_like(x2d)
        check(lib().dvq_layernorm_bwd_res_drop(_p(x2d), _p(dy), _p(dres), dt(x2d), rows, c, _p(mr), _p(gamma), _p(dx), _p(dgamma), _p(dbeta),
                                               _p(dxd), float(drop[0]), int(drop[1]) & 0xFFFFFFFFFFFFFFFF, _s()), "dvq_layernorm_bwd_res_drop")
        return dx, dxd
    check(lib().dvq_layernorm_bwd_res(_p(x2d), _p(dy), _p(dres), dt(x2d), rows, c, _p(mr), _p(gamma), _p(dx), _p(dgamma), _p(dbeta), _s()),
          "dvq_layernorm_bwd_res")
    return dx if drop is None else (dx, None)


def gelu(x):
    y = torch.empty_like(x)
    check(lib().dvq_gelu(_p(x), dt(x), x.numel(), _p(y), _s()), "dvq_gelu")
    return y


def gelu_bwd(x, dy):
    dx = torch.empty_like(x)
    check(lib().dvq_gelu_bwd(_p(x), _p(dy), dt(x), x.numel(), _p(dx), _s()), "dvq_gelu_bwd")
    return dx


def softmax_causal_(s, rows, length, tq, offset, scale):
    """in place: s <- softmax(scale * s) with the causal mask (row r sees columns <= r % tq + offset)"""
    check(lib().dvq_softmax_causal(_p(s), dt(s), rows, length, tq, offset, scale, _p(s), _s()), "dvq_softmax_causal")
    return s


def embed_gather(idx, table, out, t0, accumulate, bstride=None):
    """out[b, t0:t0+len] (+)= table[idx[b]] ; idx int64 [B,len] (or [len] with bstride=0)"""
    b, ttot, c = out.shape
    ln = idx.shape[-1]
    bs = ln if bstride is None else bstride
    check(lib().dvq_embed_gather(_p(idx), bs, _p(table), dt(out), b, ln, ttot, t0, c, int(accumulate), _p(out), _s()),
          "dvq_embed_gather")


def embed_scatter_add(idx, dout, dtable, t0, padding_idx=-1, bstride=None):
    b, ttot, c = dout.shape
    ln = idx.shape[-1]
    bs = ln if bstride is None else bstride
    check(lib().dvq_embed_scatter_add(_p(idx), bs, _p(dout), dt(dout), b, ln, ttot, t0, c, padding_idx, dtable.shape[0], _p(dtable), _s()),
          "dvq_embed_scatter_add")


def cross_entropy(logits2d, v, target, ignore_index, loss_sum, count, gscale=None, want_grad=False):
    rows, ldl = logits2d.shape
    dl = torch.empty_like(logits2d) if want_grad else None
    check(lib().dvq_cross_entropy(_p(logits2d), dt(logits2d), rows, v, ldl, _p(target), ignore_index, _p(loss_sum), _p(count),
                                  _p(gscale), _p(dl), _s()), "dvq_cross_entropy")
    return dl


def token_nll(logits2d, v, target, ignore_index):
    """per-row negative log-likelihood (fp32, natural log) and rank of the target among the first v columns of logits2d [rows, ldl]
    (fp32 or bf16); ignored rows: nll 0, rank -1 (include/dvq_hip.h, dvq_token_nll).  -> (nll fp32 [rows], rank int32 [rows])"""
    rows, ldl = logits2d.shape
    nll = torch.empty(rows, dtype=torch.float32, device=logits2d.device)
    rank = torch.empty(rows, dtype=torch.int32, device=logits2d.device)
    check(lib().dvq_token_nll(_p(logits2d), dt(logits2d), rows, v, ldl, _p(target), ignore_index, _p(nll), _p(rank), _s()), "dvq_token_nll")
    return nll, rank


def nll_segment_sums(nll, rank, b, tp, split):
    """fp64 [b, 2, 4]: (nll sum, tokens, top-1 hits, top-5 hits) of rows [0, split) and [split, tp) of every image, rows laid out
    [b, tp]; fixed summation order (dvq_nll_segment_sums)"""
    if nll.numel() != b * tp or rank.numel() != b * tp:
        raise _lib.DvqError(f"nll_segment_sums: {nll.numel()} / {rank.numel()} rows for [{b}, {tp}]")
    out = torch.empty(b, 2, 4, dtype=torch.float64, device=nll.device)
    check(lib().dvq_nll_segment_sums(_p(nll), _p(rank), b, tp, split, _p(out), _s()), "dvq_nll_segment_sums")
    return out


def nll_cell_sums(nll, rank, pos, b, tp, split, hw1, hw2, streams, cells, outside):
    """the sums of nll_segment_sums keyed by grid cell (dvq_nll_cell_sums): pos int64 [b, tp] = the position code that decides each
    row's cell (coarse codes in rows [0, split), fine codes in [split, tp)); streams = (stream index of segment 0, of segment 1), -1
    skips a segment; written into cells fp64 [b, 4, hw1 * hw1, 4] and outside fp64 [b, 4, 4]"""
    if nll.numel() != b * tp or rank.numel() != b * tp or pos.numel() != b * tp or pos.dtype != torch.int64:
        raise _lib.DvqError(f"nll_cell_sums: {nll.numel()} / {rank.numel()} / {pos.numel()} rows ({pos.dtype}) for [{b}, {tp}]")
    if (tuple(cells.shape) != (b, 4, hw1 * hw1, 4) or tuple(outside.shape) != (b, 4, 4) or cells.dtype != torch.float64
            or outside.dtype != torch.float64 or not cells.is_contiguous() or not outside.is_contiguous()):
        raise _lib.DvqError(f"nll_cell_sums: outputs {tuple(cells.shape)} / {tuple(outside.shape)} for b={b}, hw1={hw1}")
    check(lib().dvq_nll_cell_sums(_p(nll), _p(rank), _p(pos), b, tp, split, hw1, hw2, int(streams[0]), int(streams[1]), _p(cells),
                                  _p(outside), _s()), "dvq_nll_cell_sums")


def dropout_add(x, a, p, seed):
    """x + dropout(a) in one pass (p = 0: x + a); same decisions as dropout(a, p, seed)"""
    y = torch.empty_like(x)
    check(lib().dvq_dropout_add(_p(x), _p(a), dt(x), x.numel(), float(p), int(seed) & 0xFFFFFFFFFFFFFFFF, _p(y), _s()), "dvq_dropout_add")
    return y


def dropout(x, p, seed):
    y = torch.empty_like(x)
    check(lib().dvq_dropout(_p(x), dt(x), x.numel(), float(p), int(seed) & 0xFFFFFFFFFFFFFFFF, _p(y), _s()), "dvq_dropout")
    return y


def attn_causal_ok(x, n_head, b, t):
    """do the fused attention kernels take this call (dvq_attn_causal_ok: the check the entry points make themselves)?"""
    c = x.shape[-1]
    return (x.dtype in _DT and c % n_head == 0 and rt.switch("DVQ_NO_FUSED_ATTN") != "1" and
            bool(lib().dvq_attn_causal_ok(dt(x), b, t, n_head, c // n_head)))


def _attn_scratch(q, b, t, n_head, backward):
    """scratch of an attention call, None where the kernels that run need none (forward of head sizes 128 / 256)"""
    nbytes = lib().dvq_attn_causal_scratch_bytes(b, t, n_head, q.shape[-1] // n_head, int(backward))
    return torch.empty(nbytes, dtype=torch.uint8, device=q.device) if nbytes else None


def _attn_pitch(a, b, c):
    """row pitch shared by q, k, v (or dq, dk, dv): contiguous [M, C] tensors, or column blocks of one [M, 3 C] tensor"""
    s = a.stride()
    if len(s) == 2 and s[1] == 1 and b.stride() == s and c.stride() == s and a.shape == b.shape == c.shape:
        return s[0]
    if a.is_contiguous() and b.is_contiguous() and c.is_contiguous():
        return a.shape[-1]
    raise _lib.DvqError("attention operands must be contiguous, or 2-d column blocks that share one row pitch")


def attn_causal_drop_mask(q, b, t, n_head):
    """buffer for the forward's dropout keep decisions (1 bit per score of the causal tiles; csrc/attn_common.h: drop_tile)"""
    return torch.empty(lib().dvq_attn_causal_mask_bytes(b, t, n_head) // 8, dtype=torch.int64, device=q.device)


def attn_causal_fwd(q, k, v, b, t, n_head, scale, p_drop=0.0, seed=0, drop_mask=None):
    """q, k, v [B*T, C], contiguous or column blocks of ONE projection output [B*T, 3 C] (no copies: the kernels take the row pitch; head
    size 128) -> (out [B*T, C], lse fp32 [B, n_head, T]); drop_mask (attn_causal_drop_mask): receives the keep decisions"""
    ld = _attn_pitch(q, k, v)
    out = torch.empty(q.shape, dtype=q.dtype, device=q.device)
    lse = torch.empty(b, n_head, t, dtype=torch.float32, device=q.device)
    scratch = _attn_scratch(q, b, t, n_head, False)
    c = q.shape[-1]
    _timed("attn_causal_fwd", 2 * b * t * t * c, 4 * q.numel() * q.element_size(), lambda: check(
        lib().dvq_attn_causal_fwd(_praw(q), _praw(k), _praw(v), ld, dt(q), b, t, n_head, c // n_head, float(scale), float(p_drop),
                                  int(seed) & 0xFFFFFFFFFFFFFFFF, _p(out), _p(lse), _p(scratch), _p(drop_mask), _s()),
        "dvq_attn_causal_fwd"))
    return out, lse


def attn_causal_bwd(q, k, v, out, dout, lse, b, t, n_head, scale, p_drop=0.0, seed=0, drop_mask=None, grads=None):
    """drop_mask: the buffer the forward filled with the same (p_drop, seed); None: the decisions are hashed again.  grads: (dq, dk, dv)
    to write, laid out like q, k, v (column blocks of one [B*T, 3 C] matrix that one input-gradient GEMM consumes); None: new tensors"""
    ld = _attn_pitch(q, k, v)
    if grads is None:
        if ld != q.shape[-1]:
            raise _lib.DvqError("attn_causal_bwd: q, k, v with a row pitch need grads laid out like them")
        grads = tuple(torch.empty_like(q) for _ in range(3))
    if _attn_pitch(*grads) != ld or grads[0].shape != q.shape:
        raise _lib.DvqError("attn_causal_bwd: grads must share the shape and row pitch of q, k, v")
    dq, dk, dv = grads
    scratch = _attn_scratch(q, b, t, n_head, True)
    c = q.shape[-1]
    _timed("attn_causal_bwd", 5 * b * t * t * c, 8 * q.numel() * q.element_size(), lambda: check(
        lib().dvq_attn_causal_bwd(_praw(q), _praw(k), _praw(v), ld, _p(out), _p(dout), _p(lse), dt(q), b, t, n_head, c // n_head,
                                  float(scale), float(p_drop), int(seed) & 0xFFFFFFFFFFFFFFFF, _praw(dq), _praw(dk), _praw(dv),
                                  _p(scratch), _p(drop_mask), _s()),
        "dvq_attn_causal_bwd"))
    return dq, dk, dv


def attn_full_ok(q, t):
    """does the fused single-head full attention (AttnBlock) take this call (dvq_attn_full_ok)?"""
    return (q.dtype in _DT and rt.switch("DVQ_NO_FUSED_ATTNBLOCK") != "1" and
            bool(lib().dvq_attn_full_ok(dt(q), q.shape[0] // max(1, t), t, q.shape[-1])))


def attn_full_fwd(q, k, v, b, t, scale):
    """q, k, v [B*T, C] -> (out [B*T, C], lse fp32 [B, T]); softmax over ALL keys of the image (model.py:168-192)"""
    c = q.shape[-1]
    out = torch.empty_like(q)
    lse = torch.empty(b, t, dtype=torch.float32, device=q.device)
    scratch = _attn_scratch(q, b, t, 1, False)
    _timed("attn_full_fwd", 4 * b * t * t * c, 4 * q.numel() * q.element_size(), lambda: check(
        lib().dvq_attn_full_fwd(_p(q), _p(k), _p(v), dt(q), b, t, c, float(scale), _p(out), _p(lse), _p(scratch), _s()),
        "dvq_attn_full_fwd"))
    return out, lse


def attn_full_bwd(q, k, v, out, dout, lse, b, t, scale):
    c = q.shape[-1]
    dq, dk, dv = torch.empty_like(q), torch.empty_like(q), torch.empty_like(q)
    scratch = _attn_scratch(q, b, t, 1, True)
    _timed("attn_full_bwd", 10 * b * t * t * c, 8 * q.numel() * q.element_size(), lambda: check(
        lib().dvq_attn_full_bwd(_p(q), _p(k), _p(v), _p(out), _p(dout), _p(lse), dt(q), b, t, c, float(scale), _p(dq), _p(dk), _p(dv),
                                _p(scratch), _s()), "dvq_attn_full_bwd"))
    return dq, dk, dv


def decode_stack_scratch(b, c, f, device):
    """zeroed scratch of dvq_decode_stack (activations between its phases + the barrier counters it re-arms itself)"""
    return torch.zeros(lib().dvq_decode_stack_scratch_bytes(b, c, f), dtype=torch.uint8, device=device)


def decode_stack_ok(b, c, n_head, f, tmax) -> bool:
    """does dvq_decode_stack take this geometry (its own shape check)?"""
    return bool(lib().dvq_decode_stack_ok(b, c, n_head, f, tmax))


def decode_stack_status(scratch, b, c, f, reset=True):
    """synchronising read-back of the kernel's error word: raises RuntimeError when a device-wide barrier timed out (and re-arms
    the counters so that later launches are not poisoned)"""
    check(lib().dvq_decode_stack_status(_p(scratch), b, c, f, int(reset), _s()), "dvq_decode_stack_status")


def decode_stack(table_dev, n_layers, x, n_head, f, tmax, t_dev, eps, scratch, n_workgroups=0, table_host=None):
    """one token step of all blocks of a transformer (one persistent kernel, or five launches per block); x [B, C] bf16 is updated in
    place.  table_host: the ctypes array the device table was made from (kept alive by the caller)"""
    b, c = x.shape
    host = None if table_host is None else C.cast(table_host, C.c_void_p)
    check(lib().dvq_decode_stack(_p(table_dev), n_layers, b, c, n_head, f, tmax, _p(t_dev), float(eps), _p(x), _p(scratch),
                                 int(n_workgroups), host, _s()), "dvq_decode_stack")
    return x


def attn_decode_dev(q, k_new, v_new, kcache, vcache, n_head, t_dev, scale):
    """device-indexed form (graph replay): append (k_new, v_new) at cache row t_dev[0], attend over rows [0, t]"""
    b, c = q.shape
    out = torch.empty_like(q)
    check(lib().dvq_attn_decode_dev(_p(q), _p(k_new), _p(v_new), _p(kcache), _p(vcache), dt(q), b, n_head, c // n_head, _p(t_dev),
                                    kcache.shape[1], scale, _p(out), _s()), "dvq_attn_decode_dev")
    return out


def rows_dev(x, hidden, t_dev, store):
    """hidden[:, t_dev[0]] <- x (store) or x <- hidden[:, t_dev[0]]; x [B, C], hidden [B, Tmax, C]"""
    b, c = x.shape
    check(lib().dvq_rows_dev(_p(x), _p(hidden), dt(x), b, c, hidden.shape[1], _p(t_dev), int(store), _s()), "dvq_rows_dev")
    return x


def adamw_step(p, g, m, v, lr, beta1, beta2, eps, weight_decay, step):
    check(lib().dvq_adamw(_p(p), _p(g), _p(m), _p(v), p.numel(), lr, beta1, beta2, eps, weight_decay, step, _s()), "dvq_adamw")


def adamw_dev(p, g, m, v, hyper):
    """AdamW step with the hyper-parameters read from device memory (hyper fp32 [8], see include/dvq_hip.h)"""
    check(lib().dvq_adamw_dev(_p(p), _p(g), _p(m), _p(v), p.numel(), _p(hyper), _s()), "dvq_adamw_dev")


GRAD_SQNORM_CHUNK = 32768      # elements per fp64 partial of grad_sqnorm (SQNORM_CHUNK of csrc/misc.hip)


def grad_sqnorm_workspace_bytes(n) -> int:
    return int(lib().dvq_grad_sqnorm_workspace_bytes(int(n)))


def grad_stats_block(device):
    """the 32-byte statistics block of grad_sqnorm / adamw_clip_dev (include/dvq_hip.h) before any step: norm 0, coef 1, finite,
    skipped 0"""
    return torch.tensor([0, 0, 0x3F800000, 1, 0, 0, 0, 0], dtype=torch.int32, device=device)


def grad_sqnorm(g, workspace, gstat, clip=0.0, skip_nonfinite=False):
    """gstat <- {norm, clip coefficient, finite flag, skipped count} of the flat fp32 gradient buffer g; two launches, no host read"""
    assert g.dtype == torch.float32 and gstat.dtype == torch.int32 and gstat.numel() == 8
    check(lib().dvq_grad_sqnorm(_p(g), g.numel(), float(clip), int(bool(skip_nonfinite)), _p(workspace),
                                workspace.numel() * workspace.element_size(), _p(gstat), _s()), "dvq_grad_sqnorm")
    return gstat


def read_grad_stats(gstat) -> dict:
    """host copy of a statistics block (synchronises: never inside a step)"""
    h = gstat.cpu()
    return {"norm": float(h.view(torch.float64)[0]), "coef": float(h.view(torch.float32)[2]), "finite": bool(int(h[3])),
            "skipped": int(h[4])}


def adamw_clip_dev(p, g, m, v, hyper, gstat):
    """adamw_dev on g * coef, skipped when the guard of grad_sqnorm said so (coef / skip read from gstat on the device)"""
    check(lib().dvq_adamw_clip_dev(_p(p), _p(g), _p(m), _p(v), p.numel(), _p(hyper), _p(gstat), _s()), "dvq_adamw_clip_dev")


def ema_update(e, p, rec, gstat=None):
    """e <- e - rec[0] * (e - p) over flat fp32 buffers; rec[0] = 1 - decay lives in device memory (replay-safe), gstat: the guard's
    statistics block or None -- a step the guard skipped leaves e untouched (docs/design/20-weight-ema.md)"""
    assert e.dtype == torch.float32 and p.dtype == torch.float32 and rec.dtype == torch.float32 and e.numel() == p.numel()
    assert e.is_contiguous() and p.is_contiguous() and rec.numel() >= 1
    check(lib().dvq_ema_update(_p(e), _p(p), e.numel(), _p(rec), _p(gstat) if gstat is not None else None, _s()), "dvq_ema_update")
    return e


def swap_f32(a, b):
    """exchange the contents of two non-overlapping flat fp32 buffers in one launch (no temporary)"""
    assert a.dtype == torch.float32 and b.dtype == torch.float32 and a.numel() == b.numel()
    assert a.is_contiguous() and b.is_contiguous()
    check(lib().dvq_swap_f32(_p(a), _p(b), a.numel(), _s()), "dvq_swap_f32")


# ---- per-segment statistics (docs/design/24-norm-tracking.md) ------------------------------------------------------------------
class SegmentPlan:
    """the segment table of segment_stats: `offsets` (S + 1 ascending element offsets, 0 .. n) as the host array the library checks on
    every call, and the plan the library built from it -- offsets, first chunk of each segment, one record per chunk -- in device
    memory.  Built once at set-up; a bad table raises DvqError (DVQ_ESHAPE)."""

    def __init__(self, offsets, device):
        offs = [int(o) for o in offsets]
        self.S, self.n = len(offs) - 1, (offs[-1] if offs else 0)
        self.offsets = (C.c_int64 * max(1, len(offs)))(*offs)
        nbytes = int(lib().dvq_segment_plan_bytes(self.offsets, self.S, self.n))
        if nbytes == 0:
            raise _lib.DvqError(f"segment plan: {self.S} segments over {self.n} elements: the offsets must rise from 0 to n in steps >= 1 (DVQ_ESHAPE)")
        host = torch.empty(nbytes // 8, dtype=torch.int64)
        check(lib().dvq_segment_plan_build(self.offsets, self.S, self.n, C.c_void_p(host.data_ptr()), nbytes), "dvq_segment_plan_build")
        self.nchunks = int(host[2])
        self.plan = host.to(device)

    @property
    def plan_bytes(self):
        return self.plan.numel() * 8


def segment_stats_workspace(n, S, device):
    """the chunk partials of segment_stats for any table of S segments over n elements; passes on one stream may share it"""
    return torch.empty(int(lib().dvq_segment_stats_workspace_bytes(int(n), int(S))) // 8, dtype=torch.int64, device=device)


def segment_stats_state(S, device):
    """state block of segment_stats before any launch (include/dvq_hip.h): zero, first_bad_call = -1"""
    S = int(S)
    host = torch.zeros(int(lib().dvq_segment_stats_state_bytes(S)) // 8, dtype=torch.int64)
    host[3 * S:4 * S] = -1
    return host.to(device)


def segment_stats_views(state, S) -> dict:
    """named views of a state block, or of a host copy of one"""
    S = int(S)
    return {"sumsq": state[:S].view(torch.float64), "nonfinite": state[S:2 * S], "nonfinite_total": state[2 * S:3 * S],
            "first_bad_call": state[3 * S:4 * S], "calls": state[4 * S:5 * S], "absmax": state[5 * S:].view(torch.float32)[:S]}


def segment_stats(a, b, plan, workspace, state, sticky=False, armed=None):
    """state <- per-segment {sum of squares, abs-max, Inf / NaN count} of the flat fp32 buffer a, or of a - b (exact in fp64); two
    launches, ordered sums, no host read.  sticky: also the running counters.  armed: device int32, 0 = both launches return at once"""
    assert a.dtype == torch.float32 and a.numel() == plan.n and (b is None or (b.dtype == torch.float32 and b.numel() == plan.n))
    check(lib().dvq_segment_stats(_p(a), _p(b), plan.n, plan.offsets, plan.S, _p(plan.plan), plan.plan_bytes, _p(workspace),
                                  workspace.numel() * workspace.element_size(), _p(state), int(bool(sticky)), _p(armed), _s()),
          "dvq_segment_stats")
    return state


def copy_f32_armed(dst, src, armed=None):
    """dst <- src over flat fp32 buffers in one launch that returns at once when the device int32 `armed` is 0"""
    assert dst.dtype == torch.float32 and src.dtype == torch.float32 and dst.numel() == src.numel()
    check(lib().dvq_copy_f32_armed(_p(dst), _p(src), dst.numel(), _p(armed), _s()), "dvq_copy_f32_armed")
    return dst


def set_f32x8(dst, values):
    """dst[0:8] <- values (by-value launch arguments: safe to call with the host running many steps ahead)"""
    vals = [float(x) for x in values] + [0.0] * (8 - len(values))
    check(lib().dvq_set_f32x8(_p(dst), *vals, _s()), "dvq_set_f32x8")


_SCALAR_CODE = {torch.float32: _lib.SCALAR_F32, torch.bfloat16: _lib.SCALAR_BF16, torch.float64: _lib.SCALAR_F64,
                torch.int32: _lib.SCALAR_I32, torch.int64: _lib.SCALAR_I64}


def scalar_push_state(columns, device):
    """zeroed state block of scalar_push for `columns` columns (include/dvq_hip.h: sum fp64 | cnt int64 | bad int64 | last fp32)"""
    nbytes = int(lib().dvq_scalar_push_state_bytes(int(columns)))
    if nbytes == 0:
        raise _lib.DvqError(f"scalar_push: {columns} columns, 1 .. {_lib.SCALAR_COLUMNS_MAX} supported")
    return torch.zeros(nbytes // 4, dtype=torch.float32, device=device)


def scalar_push_views(state, columns):
    """(sum fp64, cnt int64, bad int64, last fp32) views of a state block, or of a host copy of one"""
    c = int(columns)
    return (state[:2 * c].view(torch.float64), state[2 * c:4 * c].view(torch.int64), state[4 * c:6 * c].view(torch.int64),
            state[6 * c:7 * c])


def scalar_push(values, state, columns, col0=0):
    """gather `values` -- one-element device tensors (fp32 / bf16 / fp64 / int32 / int64), Python numbers, or None for a column
    that has no value this time -- into columns col0 .. of `state`: last value, fp64 running sum and count of the finite ones, count of the others.  The addresses travel in the launch
    arguments, 64 per launch: no device pointer table, no copy; a recorded step replays with the addresses it was recorded with, so
    the tensors must stay alive (the step graph's pool keeps a captured step's)."""
    n = len(values)
    if col0 < 0 or col0 + n > int(columns):           # the library refuses the launch that crosses the end; refuse the whole call before any
        raise _lib.DvqError(f"scalar_push: columns {col0} .. {col0 + n - 1} outside a state block of {columns}")
    for lo in range(0, n, _lib.SCALAR_PUSH_MAX):
        part = values[lo:lo + _lib.SCALAR_PUSH_MAX]
        rec = _lib.ScalarRecord()
        if all(v is None for v in part):
            continue
        for i, v in enumerate(part):
            if v is None:
                rec.code[i] = _lib.SCALAR_SKIP
            elif torch.is_tensor(v):
                if v.numel() != 1 or v.dtype not in _SCALAR_CODE:
                    raise TypeError(f"scalar_push takes one-element fp32 / bf16 / fp64 / int32 / int64 tensors, got {tuple(v.shape)} {v.dtype}")
                if not v.is_cuda:
                    raise _lib.DvqError("libdvq_hip kernels need device tensors (no CPU fallback)")
                rec.addr[i], rec.code[i] = v.data_ptr(), _SCALAR_CODE[v.dtype]
            else:
                rec.addr[i], rec.code[i] = C.c_uint64.from_buffer_copy(C.c_double(float(v))).value, _lib.SCALAR_IMM
        check(lib().dvq_scalar_push(C.byref(rec), len(part), col0 + lo, int(columns), _p(state), _s()), "dvq_scalar_push")
    return state


def codebook_health(counts, k, stride, out3, total=None, out3_f64=None):
    """out3 (fp32 [3]) <- perplexity, active codes, tokens of the per-code counts counts[j * stride], j < k (fp32 or int64; the EMA
    quantiser's are column D of its [K, D + 1] statistics); total (fp64 [k]) += counts.  One workgroup, fp64, fixed order."""
    code = _SCALAR_CODE.get(counts.dtype)
    assert code in (_lib.SCALAR_F32, _lib.SCALAR_I64), f"counts are fp32 or int64, got {counts.dtype}"
    assert out3.dtype == torch.float32 and out3.numel() >= 3 and (total is None or (total.dtype == torch.float64 and total.numel() >= k))
    assert out3_f64 is None or (out3_f64.dtype == torch.float64 and out3_f64.numel() >= 3)
    assert counts.is_cuda and counts.numel() > 0
    # the counts may be a strided column of a larger buffer: the caller vouches that element j * stride past data_ptr() exists
    check(lib().dvq_codebook_health(_praw(counts), code, int(k), int(stride), _p(out3), _p(out3_f64), _p(total), _s()), "dvq_codebook_health")
    return out3


def sample_rows(k, n, state):
    """k distinct pseudo-random indices in [0, n) (device-resident RNG state uint64-as-int64 [2]: replayable in a hipGraph)"""
    out = torch.empty(k, dtype=torch.int64, device=state.device)
    check(lib().dvq_sample_rows(_p(out), k, n, _p(state), _s()), "dvq_sample_rows")
    return out


def add_uniform_(x, scale, state):
    """x (fp32, contiguous) += scale * U[0,1) drawn from the device-resident generator state (replay-safe)"""
    assert x.dtype == torch.float32 and x.is_contiguous()
    check(lib().dvq_add_uniform(_p(x), x.numel(), float(scale), _p(state), _s()), "dvq_add_uniform")
    return x


def attn_decode(q, kcache, vcache, n_head, t, scale):
    """q [B,C], caches [B,Tmax,C]; attention of the newest row over the first t cache rows -> [B,C]"""
    b, c = q.shape
    out = torch.empty_like(q)
    check(lib().dvq_attn_decode(_p(q), _p(kcache), _p(vcache), dt(q), b, n_head, c // n_head, t, kcache.shape[1], scale, _p(out), _s()),
          "dvq_attn_decode")
    return out


def token_rule_ok(logits2d) -> bool:
    """can the kernels that take a token rule (sample_*, codec_*) run on these logits?  [B, V] on the device, fp32 or bf16, unit column
    stride (a column slice of a padded matrix is fine), at most DVQ_TOKEN_RULE_MAXV columns"""
    return (logits2d.is_cuda and logits2d.dtype in _DT and logits2d.dim() == 2 and logits2d.stride(1) == 1
            and logits2d.shape[1] <= _lib.TokenRule.MAXV)


def _token_rule(logits2d, pad_code, forbid_idx, forbid_from, forbid_codes, keep_code, late_forbid_code, finished):
    """dvq_token_rule of include/dvq_hip.h (the rule is described there) for the B rows of logits2d -> (the filled struct, the tensors
    it points at: alive until the call is issued).  forbid_idx int64 [>= B, L]; finished [>= B]; forbid_from None: no bound"""
    b = logits2d.shape[0]
    assert logits2d.is_cuda and logits2d.stride(1) == 1, "row-major logits (a column slice of a padded matrix is fine)"
    fi = forbid_idx.contiguous() if forbid_idx is not None and forbid_idx.shape[1] > 0 else None
    fin = finished.reshape(-1).to(torch.float32).contiguous() if finished is not None else None
    assert (fi is None or (fi.dtype == torch.int64 and fi.shape[0] >= b)) and (fin is None or fin.numel() >= b)
    n_forbid, ld = (fi.shape[1], fi.stride(0)) if fi is not None else (0, 0)
    codes = (C.c_int64 * 4)(*([int(c) for c in forbid_codes] + [-1] * (4 - len(forbid_codes))))
    return _lib.TokenRule(_p(fi), n_forbid, ld, -1 if forbid_from is None else int(forbid_from), codes, int(keep_code),
                          int(late_forbid_code), int(pad_code), _p(fin)), (fi, fin)


def _logits_args(logits2d):
    """(logits, dtype, B, V, ldl): the leading arguments of the entry points that take one row of logits2d per token"""
    b, v = logits2d.shape
    return _praw(logits2d), dt(logits2d), b, v, logits2d.stride(0)


def sample_constrained(logits2d, temperature, pad_code, state, forbid_idx=None, forbid_from=None, forbid_codes=(), keep_code=-1,
                       late_forbid_code=-1, finished=None, top_k=None, top_p=None, sample=True):
    """one token per row of logits2d [B, V] (token_rule_ok) under Dualformer's constraint rule (_token_rule), top-k / top-p, multinomial
    or top-1: ONE launch (csrc/transformer.hip: dvq_sample_constrained).  state = int64 [2] device generator state (key, counter).
    -> int64 [B, 1]"""
    out = torch.empty(logits2d.shape[0], 1, dtype=torch.int64, device=logits2d.device)
    rule, keep = _token_rule(logits2d, pad_code, forbid_idx, forbid_from, forbid_codes, keep_code, late_forbid_code, finished)
    check(lib().dvq_sample_constrained(*_logits_args(logits2d), float(temperature), C.byref(rule), int(top_k or 0), float(top_p or 0.0),
                                       int(bool(sample)), _p(state), _p(out), _s()), "dvq_sample_constrained")
    return out


def sample_guided(logits2d, guidance, temperature, pad_code, state, forbid_idx=None, forbid_from=None, forbid_codes=(), keep_code=-1,
                  late_forbid_code=-1, finished=None, top_k=None, top_p=None, sample=True):
    """classifier-free-guided sample_constrained (csrc/transformer.hip: dvq_sample_guided): logits2d [2B, V], rows [0, B) conditional,
    rows [B, 2B) unconditional; the pipeline runs on fmaf(1 - guidance, u, guidance * c) per pair.  forbid_idx / finished are the
    2B-row tensors (rows [0, B) are read).  -> int64 [2B, 1], the pair's token in row i and row i + B"""
    b2, v = logits2d.shape
    assert b2 % 2 == 0, "guided sampling takes [conditional ; unconditional] rows"
    out = torch.empty(b2, 1, dtype=torch.int64, device=logits2d.device)
    rule, keep = _token_rule(logits2d, pad_code, forbid_idx, forbid_from, forbid_codes, keep_code, late_forbid_code, finished)
    check(lib().dvq_sample_guided(_praw(logits2d), dt(logits2d), b2 // 2, v, logits2d.stride(0), float(guidance), float(temperature),
                                  C.byref(rule), int(top_k or 0), float(top_p or 0.0), int(bool(sample)), _p(state), _p(out), _s()),
          "dvq_sample_guided")
    return out


# ---------------------------------------------------------------------------------------------
# lossless token codec (csrc/codec.hip, docs/design/27-token-codec.md)
# ---------------------------------------------------------------------------------------------
CODEC_PREC, CODEC_M, CODEC_L = 16, 1 << 16, 1 << 31
CODEC_ERRORS = {1: "a token the model's rule forbids (frequency 0)", 2: "a read past the end of a word stream",
                4: "a live row with no allowed symbol", 8: "no symbol under the coder's state"}


def codec_tables(logits2d, pad_code, forbid_idx=None, forbid_from=None, forbid_codes=(), keep_code=-1, late_forbid_code=-1,
                 finished=None):
    """the codec's integer frequency table of every row of logits2d [B, V] (token_rule_ok) under a constraint rule (the rule arguments
    of sample_constrained): int32 [B, V], sum 65536 per row (dvq_codec_tables; for tests and inspection)"""
    out = torch.empty(logits2d.shape, dtype=torch.int32, device=logits2d.device)
    rule, keep = _token_rule(logits2d, pad_code, forbid_idx, forbid_from, forbid_codes, keep_code, late_forbid_code, finished)
    check(lib().dvq_codec_tables(*_logits_args(logits2d), C.byref(rule), _p(out), _s()), "dvq_codec_tables")
    return out


def codec_record(logits2d, target, records, step, err, pad_code, forbid_idx=None, forbid_from=None, forbid_codes=(), keep_code=-1,
                 late_forbid_code=-1, finished=None):
    """records[:, step] (int32 [B, T]) = cum | f << 16 of target (int64 [B] or [B, 1]) under the row's table, 0 where the step codes
    nothing; err int32 [B] collects error bits (CODEC_ERRORS).  -> int64 [B, 1], the token to feed onwards (dvq_codec_record)"""
    b = logits2d.shape[0]
    out = torch.empty(b, 1, dtype=torch.int64, device=logits2d.device)
    tg = target.reshape(-1).contiguous()
    assert tg.dtype == torch.int64 and tg.numel() == b and records.dtype == torch.int32 and records.shape[0] == b
    assert records.stride(1) == 1
    assert err.dtype == torch.int32 and err.numel() == b and err.is_contiguous() and 0 <= step < records.shape[1]
    rule, keep = _token_rule(logits2d, pad_code, forbid_idx, forbid_from, forbid_codes, keep_code, late_forbid_code, finished)
    check(lib().dvq_codec_record(*_logits_args(logits2d), C.byref(rule), _p(tg), _p(records), records.stride(0), int(step), _p(out),
                                 _p(err), _s()), "dvq_codec_record")
    return out


def codec_encode(records, steps, counts=None, kinds=None, want_bits=False):
    """rANS-code the first `steps` records of every row of records int32 [B, T] (counts int64 [B]: fewer for some rows), last to first.
    -> (words int32 [B, steps + 2], nwords int64 [B], bits fp64 [B, 3] or None): row b's stream is words[b, steps + 2 - nwords[b]:];
    bits = sum of log2(M / f) over the coded steps by kinds[step] (uint8 [steps], values 0 .. 2)"""
    b = records.shape[0]
    assert records.dtype == torch.int32 and records.stride(1) == 1 and 0 <= steps <= records.shape[1]
    dev = records.device
    cap = steps + 2
    words = torch.zeros(b, cap, dtype=torch.int32, device=dev)
    nwords = torch.empty(b, dtype=torch.int64, device=dev)
    bits = torch.empty(b, 3, dtype=torch.float64, device=dev) if want_bits else None
    if counts is not None:
        counts = counts.reshape(-1).to(torch.int64).contiguous()
        assert counts.numel() == b
    if kinds is not None:
        kinds = kinds.reshape(-1).to(torch.uint8).contiguous()
        assert kinds.numel() >= steps
    check(lib().dvq_codec_encode(_p(records), b, steps, records.stride(0), _p(counts), _p(kinds), _p(words), cap, _p(nwords), _p(bits),
                                 _s()), "dvq_codec_encode")
    return words, nwords, bits


def codec_decode_state(words, base, count):
    """the decoder's per-row state int64 [B, 4] = {rANS state, cursor, first word, word count} for streams laid out in `words` (int32,
    flat) at base[b] .. base[b] + count[b] (int64 [B]; every count >= 2 and every stream inside `words`: the caller has checked)"""
    w = words.reshape(-1)
    base, count = base.reshape(-1).to(torch.int64), count.reshape(-1).to(torch.int64)
    lo = w[base].to(torch.int64) & 0xFFFFFFFF
    hi = w[base + 1].to(torch.int64) & 0xFFFFFFFF
    return torch.stack([lo | (hi << 32), torch.full_like(base, 2), base, count], dim=1).contiguous()


def codec_decode_step(logits2d, state, words, err, pad_code, forbid_idx=None, forbid_from=None, forbid_codes=(), keep_code=-1,
                      late_forbid_code=-1, finished=None):
    """one token per row from the rows' rANS states (codec_decode_state) under the rows' tables; the states advance and refill from
    `words` with the cursor bounds-checked (dvq_codec_decode_step).  -> int64 [B, 1]"""
    b = logits2d.shape[0]
    out = torch.empty(b, 1, dtype=torch.int64, device=logits2d.device)
    assert state.dtype == torch.int64 and state.shape == (b, 4) and state.is_contiguous()
    assert words.dtype == torch.int32 and words.is_contiguous() and err.dtype == torch.int32 and err.numel() == b and err.is_contiguous()
    rule, keep = _token_rule(logits2d, pad_code, forbid_idx, forbid_from, forbid_codes, keep_code, late_forbid_code, finished)
    check(lib().dvq_codec_decode_step(*_logits_args(logits2d), C.byref(rule), _p(state), _p(words), words.numel(), _p(out), _p(err), _s()),
          "dvq_codec_decode_step")
    return out


def label_dropout(labels, p, null_label, seed):
    """int64 [B] class labels -> labels with each replaced by null_label with probability p (dvq_label_dropout: dvq_dropout's hash of
    (seed, element index), so a seed reproduces the decisions)"""
    lab = labels.reshape(-1).to(torch.int64).contiguous()
    out = torch.empty_like(lab)
    if lab.numel() == 0:
        return out.view(labels.shape)
    check(lib().dvq_label_dropout(_p(lab), lab.numel(), float(p), int(null_label), int(seed) & 0xFFFFFFFFFFFFFFFF, _p(out), _s()),
          "dvq_label_dropout")
    return out.view(labels.shape)


# ---------------------------------------------------------------------------------------------
# reconstruction evaluation (csrc/metrics.hip)
# ---------------------------------------------------------------------------------------------
def recon_metrics_workspace(b, h, w, device):
    """uint8 workspace of dvq_recon_metrics_workspace_bytes(b, h, w) bytes (per-tile partial sums)"""
    return torch.empty(int(lib().dvq_recon_metrics_workspace_bytes(b, h, w)), dtype=torch.uint8, device=device)


def recon_metrics(x, y, quantize_u8=False, ws=None, out=None):
    """x (target), y (reconstruction) NCHW fp32 [B,3,H,W] in [-1, 1] -> (mse, l1, ssim), fp64 [B] each (definitions:
    include/dvq_hip.h, dvq_recon_metrics).  ws: recon_metrics_workspace(B, H, W) or None (allocated here); out: three fp64 [B]
    tensors to write into, or None"""
    b, c, h, w = x.shape
    assert c == 3 and x.dtype == torch.float32 and y.dtype == torch.float32 and tuple(y.shape) == tuple(x.shape)
    if ws is None:
        ws = recon_metrics_workspace(b, h, w, x.device)
    mse, l1, ssim = out if out is not None else [torch.empty(b, dtype=torch.float64, device=x.device) for _ in range(3)]
    check(lib().dvq_recon_metrics(_p(x), _p(y), b, h, w, int(bool(quantize_u8)), _p(mse), _p(l1), _p(ssim), _p(ws), ws.numel(), _s()),
          "dvq_recon_metrics")
    return mse, l1, ssim


def recon_cells_workspace(b, h, w, hg, wg, device):
    """uint8 workspace of dvq_recon_cells_workspace_bytes(b, h, w, hg, wg) bytes (per-tile, per-cell-piece partial sums)"""
    return torch.empty(int(lib().dvq_recon_cells_workspace_bytes(b, h, w, hg, wg)), dtype=torch.uint8, device=device)


def recon_cells(x, y, hg, wg, quantize_u8=False, ws=None):
    """x (target), y (reconstruction) NCHW fp32 [B,3,H,W] in [-1, 1] over an hg x wg cell grid -> fp64 [B, hg, wg, 3]: per cell the SUMS
    of (x01 - y01)^2, of |x - y| and of the SSIM index of the windows whose top-left pixel lies in the cell (include/dvq_hip.h,
    dvq_recon_cells).  ws: recon_cells_workspace(B, H, W, hg, wg) or None (allocated here)"""
    b, c, h, w = x.shape
    assert c == 3 and x.dtype == torch.float32 and y.dtype == torch.float32 and tuple(y.shape) == tuple(x.shape)
    assert x.is_contiguous() and y.is_contiguous()
    if ws is None:
        ws = recon_cells_workspace(b, h, w, hg, wg, x.device)
    cells = torch.empty(b, max(int(hg), 0), max(int(wg), 0), 3, dtype=torch.float64, device=x.device)     # (a bad grid: the library says so)
    check(lib().dvq_recon_cells(_p(x), _p(y), b, h, w, hg, wg, int(bool(quantize_u8)), _p(cells), _p(ws), ws.numel(), _s()),
          "dvq_recon_cells")
    return cells


def code_histogram(codes, grain, n_codes, n_grains, counts, invalid, tokens=None):
    """codes int64 [B,Hf,Wf], grain int64 [B,hg,wg] or None (n_grains = 1); counts int64 [n_grains, n_codes] and invalid int64 [1]
    are ACCUMULATED (zero them once).  -> tokens int64 [B] (tokens per image by the grain's alignment rule, include/dvq_hip.h)"""
    b, hf, wf = codes.shape
    assert codes.dtype == torch.int64 and counts.dtype == torch.int64 and invalid.dtype == torch.int64
    assert tuple(counts.shape) == (n_grains, n_codes) and invalid.numel() >= 1
    hg = wg = 0
    if grain is not None:
        assert grain.dtype == torch.int64 and grain.shape[0] == b
        hg, wg = grain.shape[1], grain.shape[2]
    if tokens is None:
        tokens = torch.empty(b, dtype=torch.int64, device=codes.device)
    check(lib().dvq_code_histogram(_p(codes), _p(grain), b, hf, wf, hg, wg, int(n_codes), int(n_grains), _p(counts), _p(tokens),
                                   _p(invalid), _s()), "dvq_code_histogram")
    return tokens


# ---------------------------------------------------------------------------------------------
# sample-set metrics (csrc/sampleset.hip, docs/design/32-sample-set-metrics.md)
# ---------------------------------------------------------------------------------------------
def _feature_rows(name, t):
    """fp32 [N, D] rows of any pitch (a column slice of a wider contiguous matrix passes) -> (N, D, pitch)"""
    if not torch.is_tensor(t) or t.dtype != torch.float32 or t.dim() != 2:
        raise TypeError(f"{name}: expected an fp32 [N, D] tensor")
    n, d = int(t.shape[0]), int(t.shape[1])
    if n and d and (t.stride(1) != 1 or (n > 1 and t.stride(0) < d)):
        raise _lib.DvqError(f"{name}: rows must be contiguous (strides {t.stride()})")
    return n, d, int(t.stride(0)) if n > 1 else max(d, 1)


def feat_moments(x, shift, out=None):
    """x fp32 [N, D] (rows of any pitch), shift fp32 [D] -> (sum fp64 [D], gram fp64 [D, D] upper triangle, n int64 [1]) of
    fl32(x - shift), ACCUMULATED into `out` (the three tensors of an earlier call) or into fresh zeros (include/dvq_hip.h,
    dvq_feat_moments).  The lower triangle of gram is never written: mirror it on the host."""
    n, d, ld = _feature_rows("feat_moments: x", x)
    assert shift.dtype == torch.float32 and shift.numel() == d
    if out is None:
        out = (torch.zeros(d, dtype=torch.float64, device=x.device), torch.zeros(d, d, dtype=torch.float64, device=x.device),
               torch.zeros(1, dtype=torch.int64, device=x.device))
    s, g, cnt = out
    assert s.dtype == torch.float64 and g.dtype == torch.float64 and cnt.dtype == torch.int64 and tuple(g.shape) == (d, d) and s.numel() == d
    check(lib().dvq_feat_moments(_praw(x), n, d, ld, _p(shift), _p(s), _p(g), _p(cnt), _s()), "dvq_feat_moments")
    return s, g, cnt


def pair_scan_workspace(na, nb, k, device):
    """uint8 workspace of dvq_pair_scan_workspace_bytes(na, nb, k) bytes (per-split candidate lists; empty when b is not split)"""
    return torch.empty(int(lib().dvq_pair_scan_workspace_bytes(na, nb, k)), dtype=torch.uint8, device=device)


def pair_scan(a, b, k, rad2_b=None, exclude_diag=False, ws=None, count=None):
    """a fp32 [Na, D], b fp32 [Nb, D] (rows of any pitch; CENTRED features) -> (kth2 fp32 [Na, k], idx int64 [Na, k], count int64 [Na] or
    None): per row of a its k smallest squared distances to rows of b, their indices, and with rad2_b fp32 [Nb] the number of j with
    d2(i, j) <= rad2_b[j] (include/dvq_hip.h, dvq_pair_scan).  ws: pair_scan_workspace(Na, Nb, k) or None (allocated here)"""
    na, d, lda = _feature_rows("pair_scan: a", a)
    nb, db, ldb = _feature_rows("pair_scan: b", b)
    if d != db:
        raise _lib.DvqError(f"pair_scan: a has {d} columns, b has {db}")
    k = int(k)
    if ws is None:
        ws = pair_scan_workspace(na, nb, k, a.device)
    kth2 = torch.empty(na, max(k, 0), dtype=torch.float32, device=a.device)
    idx = torch.empty(na, max(k, 0), dtype=torch.int64, device=a.device)
    if rad2_b is not None:
        assert rad2_b.dtype == torch.float32 and rad2_b.numel() == nb
        if count is None:
            count = torch.empty(na, dtype=torch.int64, device=a.device)
    check(lib().dvq_pair_scan(_praw(a), lda, _praw(b), ldb, na, nb, d, _p(rad2_b), k, int(bool(exclude_diag)), _p(kth2), _p(idx),
                              _p(count), _p(ws) if ws.numel() else None, ws.numel(), _s()), "dvq_pair_scan")
    return kth2, idx, count


# ---------------------------------------------------------------------------------------------
# token shards (csrc/tokens.hip, docs/design/16-token-shards.md)
# ---------------------------------------------------------------------------------------------
def _tokens_arg(name, t, dtype, shape):
    if not torch.is_tensor(t) or t.dtype != dtype:
        raise TypeError(f"{name}: expected a {dtype} tensor, got {t.dtype if torch.is_tensor(t) else type(t).__name__}")
    if tuple(t.shape) != tuple(shape):
        raise _lib.DvqError(f"{name}: expected shape {tuple(shape)}, got {tuple(t.shape)}")
    return t


def tokens_pack(indices, grain, codebook_size, out=None):
    """indices int64 [B, fhw, fhw], grain int64 [B, hw1, hw1] (DualGrainVQModel.encode's info[2] and grain map) -> (codes uint16
    [B, fhw * fhw], grain_bits uint32 [B, ceil(hw1^2 / 32)], n_fine_cells int32 [B], bad int32 [B]); definitions: include/dvq_hip.h,
    dvq_tokens_pack.  out: the four tensors to write into, or None.  Never synchronises: the caller reads `bad`."""
    if not torch.is_tensor(indices) or indices.dtype != torch.int64 or indices.dim() != 3 or indices.shape[1] != indices.shape[2]:
        raise TypeError("tokens_pack: indices must be an int64 [B, fhw, fhw] tensor")
    b, fhw = int(indices.shape[0]), int(indices.shape[1])
    if not torch.is_tensor(grain) or grain.dtype != torch.int64 or grain.dim() != 3 or grain.shape[1] != grain.shape[2]:
        raise TypeError("tokens_pack: grain must be an int64 [B, hw1, hw1] tensor")
    hw1 = int(grain.shape[1])
    if grain.shape[0] != b or hw1 == 0 or fhw % hw1:
        raise _lib.DvqError(f"tokens_pack: grain {tuple(grain.shape)} does not tile indices {tuple(indices.shape)}")
    if grain.device != indices.device:
        raise _lib.DvqError("tokens_pack: indices and grain live on different devices")
    words = (hw1 * hw1 + 31) // 32
    dev = indices.device
    if out is None:
        out = (torch.empty(b, fhw * fhw, dtype=torch.uint16, device=dev), torch.empty(b, words, dtype=torch.uint32, device=dev),
               torch.empty(b, dtype=torch.int32, device=dev), torch.empty(b, dtype=torch.int32, device=dev))
    codes = _tokens_arg("tokens_pack: codes", out[0], torch.uint16, (b, fhw * fhw))
    bits = _tokens_arg("tokens_pack: grain_bits", out[1], torch.uint32, (b, words))
    n_fine = _tokens_arg("tokens_pack: n_fine_cells", out[2], torch.int32, (b,))
    bad = _tokens_arg("tokens_pack: bad", out[3], torch.int32, (b,))
    check(lib().dvq_tokens_pack(_p(indices), _p(grain), b, hw1, fhw // hw1, int(codebook_size), _p(codes), _p(bits), _p(n_fine), _p(bad),
                                _s()), "dvq_tokens_pack")
    return codes, bits, n_fine, bad


def tokens_unpack(codes, grain_bits, hw1, hw2, order, codes6, lc, lf, n_fine_cells, out=None):
    """codes uint16 [B, (hw1 * hw2)^2], grain_bits uint32 [B, ceil(hw1^2 / 32)] -> DualGrainSeperatePermuter.forward's dict (four int64
    streams [B, lc] / [B, lf] from dvq_tokens_unpack, segments of zeros / ones).  order: "region-first" | "row-first"; codes6: (content
    pad, content eos, coarse-position pad, eos, fine-position pad, eos).  n_fine_cells: the HOST's fine-cell count per image (sequence
    of ints -- the caller has the bitmap): lc < max(coarse cells) + 1 or lf < max(fine codes) + 1 raises ValueError before anything is
    launched.  out: the four stream tensors to write into, or None.  Never synchronises."""
    if order not in ("region-first", "row-first"):
        raise ValueError(f"tokens_unpack: order {order!r} is neither 'region-first' nor 'row-first'")
    if len(codes6) != 6:
        raise ValueError("tokens_unpack: codes6 = (content pad, content eos, coarse-position pad, eos, fine-position pad, eos)")
    hw1, hw2, lc, lf = int(hw1), int(hw2), int(lc), int(lf)
    ncell, q = hw1 * hw1, hw2 * hw2
    if not torch.is_tensor(codes) or codes.dtype != torch.uint16:
        raise TypeError(f"tokens_unpack: codes must be a uint16 tensor, got {getattr(codes, 'dtype', type(codes).__name__)}")
    if not torch.is_tensor(grain_bits) or grain_bits.dtype != torch.uint32:
        raise TypeError(f"tokens_unpack: grain_bits must be a uint32 tensor, got {getattr(grain_bits, 'dtype', type(grain_bits).__name__)}")
    b = int(codes.shape[0])
    _tokens_arg("tokens_unpack: codes", codes, torch.uint16, (b, ncell * q))
    _tokens_arg("tokens_unpack: grain_bits", grain_bits, torch.uint32, (b, (ncell + 31) // 32))
    if grain_bits.device != codes.device:
        raise _lib.DvqError("tokens_unpack: codes and grain_bits live on different devices")
    counts = [int(n) for n in n_fine_cells]
    if len(counts) != b or any(n < 0 or n > ncell for n in counts):
        raise ValueError(f"tokens_unpack: n_fine_cells must hold {b} counts in [0, {ncell}]")
    need_c, need_f = ncell - min(counts) + 1, max(counts) * q + 1
    if lc < need_c or lf < need_f:
        raise ValueError(f"tokens_unpack: row lengths ({lc}, {lf}) cut a stream: the batch needs at least ({need_c}, {need_f})")
    dev = codes.device
    if out is None:
        out = (torch.empty(b, lc, dtype=torch.int64, device=dev), torch.empty(b, lc, dtype=torch.int64, device=dev),
               torch.empty(b, lf, dtype=torch.int64, device=dev), torch.empty(b, lf, dtype=torch.int64, device=dev))
    cc = _tokens_arg("tokens_unpack: coarse_content", out[0], torch.int64, (b, lc))
    cp = _tokens_arg("tokens_unpack: coarse_position", out[1], torch.int64, (b, lc))
    fc = _tokens_arg("tokens_unpack: fine_content", out[2], torch.int64, (b, lf))
    fp = _tokens_arg("tokens_unpack: fine_position", out[3], torch.int64, (b, lf))
    check(lib().dvq_tokens_unpack(_p(codes), _p(grain_bits), b, hw1, hw2, 0 if order == "region-first" else 1, *[int(v) for v in codes6],
                                  lc, lf, _p(cc), _p(cp), _p(fc), _p(fp), _s()), "dvq_tokens_unpack")
    return {"coarse_content": cc, "fine_content": fc, "coarse_position": cp, "fine_position": fp,
            "coarse_segment": torch.zeros_like(cc), "fine_segment": torch.ones_like(fc)}


# ---------------------------------------------------------------------------------------------
# training-time image logging (csrc/imagelog.hip, docs/design/18-image-logging.md)
# ---------------------------------------------------------------------------------------------
def imagelog_workspace(segments, device):
    """uint8 workspace of dvq_imagelog_workspace_bytes(segments) bytes (partial minima / maxima; segments = batch size for the overlay,
    1 for the grid)"""
    return torch.empty(int(lib().dvq_imagelog_workspace_bytes(int(segments))), dtype=torch.uint8, device=device)


def _grain_args(name, x, m):
    if x.dim() != 4 or x.shape[1] != 3 or x.dtype != torch.float32:
        raise _lib.DvqError(f"{name}: images must be fp32 [B,3,H,W], got {x.dtype} {tuple(x.shape)}")
    if m.dim() != 3 or m.shape[0] != x.shape[0]:
        raise _lib.DvqError(f"{name}: map must be [B,h,w] with the images' batch size, got {tuple(m.shape)} for {tuple(x.shape)}")


def grain_overlay(x, grain=None, score=None, levels=2, low=(5, 39, 175), high=(255, 0, 0), scaler=0.9, ws=None, out=None):
    """x fp32 NCHW [B,3,H,W]; grain int64 [B,h,w] (levels 2 or 3) OR score fp32 [B,h,w] in [0,1] -> fp32 [B,3,H,W] holding k / 255:
    the image normalised by its own range, blended towards the cell's colour (include/dvq_hip.h, dvq_grain_overlay)"""
    m = grain if grain is not None else score
    if (grain is None) == (score is None):
        raise _lib.DvqError("grain_overlay: pass a grain map or a score map, not both or neither")
    _grain_args("grain_overlay", x, m)
    if m.dtype != (torch.int64 if grain is not None else torch.float32):
        raise TypeError(f"grain_overlay: a grain map is int64, a score map fp32; got {m.dtype}")
    b, _, hh, ww = x.shape
    if ws is None:
        ws = imagelog_workspace(b, x.device)
    if out is None:
        out = torch.empty_like(x)
    rgb = [(int(c[0]) << 16) | (int(c[1]) << 8) | int(c[2]) for c in (low, high)]
    check(lib().dvq_grain_overlay(_p(x), _p(grain), _p(score), int(levels), b, hh, ww, m.shape[1], m.shape[2], rgb[0], rgb[1],
                                  float(scaler), _p(out), _p(ws), ws.numel(), _s()), "dvq_grain_overlay")
    return out


def grain_lines_(x, grain, levels):
    """in place: -1 on the cell borders and the subdivision lines of grain >= 1 (and == 2) cells; x fp32 [B,3,H,W], grain int64 [B,h,w]"""
    _grain_args("grain_lines_", x, grain)
    if grain.dtype != torch.int64:
        raise TypeError(f"grain_lines_: the grain map is int64, got {grain.dtype}")
    b, _, hh, ww = x.shape
    check(lib().dvq_grain_lines(_p(x), _p(grain), int(levels), b, hh, ww, grain.shape[1], grain.shape[2], _s()), "dvq_grain_lines")
    return x


def image_grid_shape(n, h, w, nrow=4, padding=2):
    gh, gw = C.c_int64(0), C.c_int64(0)
    check(lib().dvq_image_grid_shape(int(n), int(h), int(w), int(nrow), int(padding), C.byref(gh), C.byref(gw)), "dvq_image_grid_shape")
    return int(gh.value), int(gw.value)


def image_grid_u8(x, nrow=4, padding=2, clamp=True, ws=None, out=None):
    """x fp32 [N,C,H,W], C in {1, 3} -> uint8 [GH,GW,3]: make_grid(nrow, padding, normalize=True) * 255, truncated (include/dvq_hip.h,
    dvq_image_grid_u8)"""
    if x.dim() != 4 or x.dtype != torch.float32:
        raise _lib.DvqError(f"image_grid_u8: images must be fp32 [N,C,H,W], got {x.dtype} {tuple(x.shape)}")
    n, c, hh, ww = x.shape
    gh, gw = image_grid_shape(n, hh, ww, nrow, padding)
    if ws is None:
        ws = imagelog_workspace(1, x.device)
    if out is None:
        out = torch.empty(gh, gw, 3, dtype=torch.uint8, device=x.device)
    check(lib().dvq_image_grid_u8(_p(x), n, c, hh, ww, int(nrow), int(padding), int(bool(clamp)), _p(out), out.numel(), _p(ws), ws.numel(),
                                  _s()), "dvq_image_grid_u8")
    return out
