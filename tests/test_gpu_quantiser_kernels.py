"""The quantiser's training-side kernels (csrc/vq.hip: dvq_vq_ema_stats, dvq_vq_gather_loss, dvq_vq_backward, dvq_vq_embed,
dvq_vq_ema_apply, dvq_vq_distances) and the grain merges (csrc/misc.hip: dvq_dual_merge[_bwd]; csrc/router.hip: dvq_grain_merge[_bwd],
dvq_avgpool_slice[_bwd]), called through kernels.py as the product calls them, at the smallest shapes that reach every edge of their
dispatch, compared PER ELEMENT with the float64 restatement of tests/vq_math.py.  docs/design/31-quantiser-kernel-pins.md has the
edge -> case table and the tolerances.

Operands are drawn from a seeded RandomState and rounded to the tensor type before the reference sees them.  Bounds:
  exact          gathers, selections, masks, x_q = fl(x + fl(e - x)) and its bf16 rounding, counts, zero rows: bit for bit;
  derived        (constant 1) per-code sums, the loss sum, dx, the merges' scaled values and gradients, the pools -- stated at each check;
  bf16 outputs   |got - ref| <= 2^-8 |ref| + the fp32 term: one correctly rounded bf16 store on top of the fp32 arithmetic;
  measured       |got - ref| <= K 2^-24 form (+ 2^-126): K = FP32_K[family], four times the largest ratio of the fp32 kernel against
                 the float64 reference over every case of the family in this file, both modes (FP32_MEASURED, one run on an MI355X).
"Modes": deterministic mode off and on with the same bound; with the mode on two launches are bit-identical and
kernels.unordered_launches() does not move."""
import contextlib
import functools
import math
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest
import torch

import vq_math as M

pytestmark = pytest.mark.gpu

U = 2.0 ** -24            # fp32 unit roundoff
BF = 2.0 ** -8            # bf16 unit roundoff (round to nearest even, 8 significant bits)
TINY = 2.0 ** -126        # smallest normal fp32

# largest (error - 2^-126) / (2^-24 x form) of the fp32 kernels over every case of the family in this file, both modes, one MI355X run
FP32_MEASURED = {"n_ema": 0.9725, "s_ema": 1.6, "weight": 0.2272, "distances": 0.8127, "dscale": 0.117}
# chosen: four times the measurement (other summation orders between modes and launches)
FP32_K = {family: 4.0 * worst for family, worst in FP32_MEASURED.items()}
# derived bounds carry no constant
FP32_K.update(stats=1.0, loss=1.0, dx=1.0, merge=1.0, merge_grad=1.0, pool=1.0)
CEIL_EMA = (1e-4, 1e-5)            # test_vq_ema_golden accepts rtol 1e-4 / atol 1e-5 on s_ema and weight
CEIL_DIST = (2e-5, 2e-4)           # test_vq_distances_and_soft_codes_golden accepts rtol 2e-5 / atol 2e-4
CEIL_LOSS = 1e-5                   # test_vq_forward_golden accepts rtol 1e-5 on the loss

DECAY = float(np.float32(0.99))    # the value the kernel receives (1 - DECAY is exact in fp32)
EPS = float(np.float32(1e-5))

DTYPES = pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
MODES = pytest.mark.parametrize("det", [False, True], ids=["mode-off", "deterministic"])


def _k():
    from dynamicvectorquantization_amd import kernels as K
    return K


def _err_type():
    from dynamicvectorquantization_amd._lib import DvqError
    return DvqError


@contextlib.contextmanager
def _mode(det, dev=None):
    K = _k()
    try:
        K.set_deterministic(det)
        if det and dev is not None:
            K.ensure_workspace(dev)            # the per-workgroup partials of the ordered forms live in the registered scratch
        yield K
    finally:
        K.set_deterministic(False)


def _rnd(a, dtype):
    """float64 draw -> the value the tensor type holds, as float32"""
    a = np.ascontiguousarray(a, dtype=np.float32)
    return M.bf16_round(a) if dtype == torch.bfloat16 else a


def _dev(a, dev, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return t if dtype is None else t.to(dtype)


def _host(t):
    """device tensor -> numpy (bf16 through float32: exact)"""
    t = t.detach()
    return (t.float() if t.dtype == torch.bfloat16 else t).cpu().numpy()


def _bits_equal(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, f"{what}: {got.shape} {got.dtype} against {want.shape} {want.dtype}"
    same = got.view(np.uint8) == want.view(np.uint8)
    if not bool(same.all()):
        w = int(np.argmin(same.reshape(-1))) // got.dtype.itemsize
        raise AssertionError(f"{what}: {int((~same).sum())} bytes differ; first at element {np.unravel_index(w, got.shape)}: "
                             f"got {got.reshape(-1)[w]!r} want {want.reshape(-1)[w]!r}")


def _pin(family, got, ref, form, dtype=torch.float32, ceiling=None, what=""):
    """per element: |got - ref| <= FP32_K[family] 2^-24 form + 2^-126 (+ 2^-8 |ref| for a bf16 tensor).  Prints the fp32 ratio.
    ceiling = (rtol, atol): the chosen fp32 term stays below atol + rtol |ref|, which is what assert_allclose accepts"""
    ref = np.asarray(ref, dtype=np.float64)
    got = np.asarray(got, dtype=np.float64).reshape(ref.shape)
    unit = U * np.broadcast_to(np.asarray(form, dtype=np.float64), ref.shape)
    assert bool(np.isfinite(got).all()), f"{family} {what}: non-finite output"
    err = np.abs(got - ref)
    if dtype == torch.float32 and err.size:
        over = np.maximum(err - TINY, 0.0)
        ratio = np.where(unit > 0, over / np.maximum(unit, 1e-300), np.where(over > 0, np.inf, 0.0))
        print(f"PIN {family} {float(ratio.max()):.4g} {what}")
    k = FP32_K[family]
    bound = k * unit + TINY
    if dtype == torch.bfloat16:
        bound = bound + BF * np.abs(ref)
    bad = err > bound
    if bool(bad.any()):
        w = int(np.argmax((err - bound).reshape(-1)))
        raise AssertionError(f"{family} {what}: {int(bad.sum())} of {bad.size} elements out of bound; worst at {np.unravel_index(w, err.shape)}: "
                             f"got {got.reshape(-1)[w]!r} ref {ref.reshape(-1)[w]!r} err {err.reshape(-1)[w]:.3e} bound {bound.reshape(-1)[w]:.3e}")
    if ceiling is not None and err.size:
        rtol, atol = ceiling
        top = float((k * unit / (atol + rtol * np.abs(ref))).max())
        print(f"CEIL {family} {top:.3g} {what}")
        assert top <= 1.0, f"{family} {what}: chosen fp32 bound is {top:.3g} x (atol {atol} + rtol {rtol} |ref|)"


def _tag(dtype, det):
    return f"{'bf16' if dtype == torch.bfloat16 else 'fp32'} det {int(det)}"


# ==== vq_ema_stats ========================================================================================================================
EMA_SLICE = 1024          # rows per (code, slice) work item (csrc/vq.hip)


def _stats_case(dev, x, idx, k, dtype, det, what):
    """x [N, D] (already rounded to dtype), idx [N].  Counts exact; sums |got - ref| <= (cnt_k + slices_k) 2^-24 sum|x| (a code's rows
    are added one by one in fp32, then one add per slice that holds rows of the code); a code without rows is exactly zero in every
    column, whatever the buffer held before"""
    n, d = x.shape
    sums, cnt = M.code_sums(x, idx, k)
    sabs, _ = M.code_sums(np.abs(x), idx, k)
    slices = np.zeros(k)
    for s in range(0, n, EMA_SLICE):
        slices[np.unique(idx[s:s + EMA_SLICE])] += 1
    xt, it = _dev(x, dev, dtype), _dev(idx, dev)
    with _mode(det, dev) as K:
        c0 = K.unordered_launches()
        outs = []
        for _ in range(2 if det else 1):
            out = torch.full((k, d + 1), float("nan"), device=dev)          # a fresh allocation: 16-byte aligned, as the zero fill needs
            outs.append(K.vq_ema_stats(xt, it, k, out=out))
        torch.cuda.synchronize()
        if det:
            assert torch.equal(outs[0], outs[1]), f"{what}: deterministic mode: identical launches differ"
            assert K.unordered_launches() == c0, f"{what}: deterministic mode took an unordered path"
        elif n > EMA_SLICE:
            assert K.unordered_launches() > c0, f"{what}: several slices with the mode off were not counted as unordered"
    got = _host(outs[0])
    assert np.array_equal(got[:, d], cnt), f"{what}: counts differ: {got[:, d]} against {cnt}"
    _pin("stats", got[:, :d], sums, (cnt + slices)[:, None] * sabs, what="sums " + what)
    empty = cnt == 0
    assert not bool(got[empty].any()) and not bool(np.isnan(got[empty]).any()), f"{what}: a code without rows is not zero"
    return got


def _draw_rows(n, d, dtype, seed):
    rs = np.random.RandomState(seed)
    return _rnd(1.5 * rs.standard_normal((n, d)) + 0.5, dtype), rs


STATS_D = [1, 63, 64, 65, 128, 129, 256, 257, 512, 513, 1024]


@DTYPES
@pytest.mark.parametrize("d", STATS_D)
def test_ema_stats_nj_dispatch(dev, d, dtype):
    """NJ = 1 / 2 / 4 / 8 / 16 at both sides of each threshold, lanes past the row masked: N 300 (one slice), K 5"""
    x, rs = _draw_rows(300, d, dtype, 100 + d)
    idx = rs.randint(0, 5, 300).astype(np.int64)
    for det in (False, True):                                   # one slice: the mode does not change the launch
        _stats_case(dev, x, idx, 5, dtype, det, f"D {d} {_tag(dtype, det)}")


@MODES
@DTYPES
@pytest.mark.parametrize("d", [72, 256])
@pytest.mark.parametrize("n", [1, 1023, 1024, 1025, 4096 + 7])
def test_ema_stats_slice_seams(dev, n, d, dtype, det):
    """one row; a slice one row short, full, one row into the second slice; four slices and seven rows: the clamped index loads past N.
    With the mode on N > 1024 is the ALL instantiation: one wave per code walks every slice"""
    x, rs = _draw_rows(n, d, dtype, 7 * n + d)
    idx = rs.randint(0, 7, n).astype(np.int64)
    idx[-1] = 6                                                 # the last row counts
    _stats_case(dev, x, idx, 7, dtype, det, f"N {n} D {d} {_tag(dtype, det)}")


@DTYPES
def test_ema_stats_rows_per_trip(dev, dtype):
    """four rows per trip: codes that own exactly 0, 1, 2, 3, 4, 5 rows of one slice"""
    owners = np.repeat(np.arange(6), np.arange(6)).astype(np.int64)           # 15 rows
    x, rs = _draw_rows(len(owners), 72, dtype, 41)
    idx = owners[rs.permutation(len(owners))]
    assert list(np.bincount(idx, minlength=6)) == [0, 1, 2, 3, 4, 5]
    _stats_case(dev, x, idx, 6, dtype, False, f"rows per trip {_tag(dtype, False)}")


@MODES
@DTYPES
@pytest.mark.parametrize("kind", ["full-list", "skew-70"])
def test_ema_stats_full_list_and_skew(dev, kind, dtype, det):
    """full-list: code 2 owns all 1024 rows of the second slice of three (and none elsewhere): the compact list at its capacity.
    skew-70: 70 % of 4096 rows on code 3, as test_vq_ema_statistics_ordered draws them"""
    if kind == "full-list":
        n, k, d = 3 * EMA_SLICE - 5, 5, 72
        x, rs = _draw_rows(n, d, dtype, 43)
        idx = rs.choice([0, 1, 3], n).astype(np.int64)          # code 4 owns nothing
        idx[EMA_SLICE:2 * EMA_SLICE] = 2
    else:
        n, k, d = 4096, 64, 64
        x, rs = _draw_rows(n, d, dtype, 19)
        idx = rs.randint(0, k, n).astype(np.int64)
        idx[rs.rand(n) < 0.7] = 3
    _stats_case(dev, x, idx, k, dtype, det, f"{kind} {_tag(dtype, det)}")


@pytest.mark.parametrize("k,d", [(3, 64), (5, 2), (1, 2)], ids=["K3-D64", "K5-D2", "K1-D2"])
def test_ema_stats_zero_fill_tail(dev, k, d):
    """K (D + 1) 4 bytes is no multiple of 16: the bulk fill stores 16 bytes at a time and a second launch zeroes the last floats.
    (1, 2) is 12 bytes: no bulk at all (the launcher once sent a grid of zero workgroups there and returned an error).  The buffer
    starts as NaN; the last code owns no row and must read as zeros"""
    assert (k * (d + 1) * 4) % 16 != 0
    n = 10
    x, rs = _draw_rows(n, d, torch.float32, 50 + k)
    idx = rs.randint(0, max(k - 1, 1), n).astype(np.int64)          # K > 1: the last code owns no row
    got = _stats_case(dev, x, idx, k, torch.float32, False, f"zero-fill tail K {k} D {d}")
    assert np.isfinite(got).all()
    if k > 1:
        assert not got[k - 1].any()


def test_ema_stats_rejects_wide_rows(dev):
    """D = 1025 > 1024: DvqError before any launch (the output keeps its fill)"""
    K = _k()
    x = torch.zeros(4, 1025, device=dev)
    out = torch.full((2, 1026), 7.0, device=dev)
    with pytest.raises(_err_type()):
        K.vq_ema_stats(x, torch.zeros(4, dtype=torch.int64, device=dev), 2, out=out)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())


# ==== vq_gather_loss, vq_backward, vq_embed ============================================================================================
MASK_VALUES = np.array([1.0, 0.25, 0.0625, 0.0], dtype=np.float32)
COEFS = (0.37, -1.25)


@functools.lru_cache(maxsize=4)
def _gather_operands(rows, d, k, bf16, masked):
    dtype = torch.bfloat16 if bf16 else torch.float32
    rs = np.random.RandomState(rows + 31 * d + k)
    x = _rnd(1.5 * rs.standard_normal((rows, d)) + 0.25, dtype)
    g = _rnd(rs.standard_normal((rows, d)), dtype)
    e = (1.5 * rs.standard_normal((k, d))).astype(np.float32)
    idx = rs.randint(0, k, rows).astype(np.int64)
    idx[0] = k - 1                                              # the codebook's last row, and its first
    if rows > 1:
        idx[-1] = 0
    mask = rs.choice(MASK_VALUES, rows).astype(np.float32) if masked else None
    return x, g, e, idx, mask


def _gather_case(dev, rows, d, k, dtype, masked, det, ceiling=False):
    """x_q and the gathers bit for bit; the loss sum within (ceil(D / 64) + 8) 2^-24 sum_n |m_n| r_n -- the rounding of e - x twice in
    its square, a lane's ceil(D / 64) fused adds, six levels of the wave's tree, the product with m; the fp64 adds behind them are below
    N 2^-53; dx within 2^-24 (2 |coef m| |x - e| + |ref|) -- one rounding of the difference, one of coef m, one of the fused
    multiply-add"""
    x, g, e, idx, mask = _gather_operands(rows, d, k, dtype == torch.bfloat16, masked)
    what = f"rows {rows} D {d} K {k} mask {int(masked)} {_tag(dtype, det)}"
    xt, gt, et, it = _dev(x, dev, dtype), _dev(g, dev, dtype), _dev(e, dev), _dev(idx, dev)
    mt = None if mask is None else _dev(mask, dev)
    coefs = [torch.tensor([c], dtype=torch.float32, device=dev) for c in COEFS]
    with _mode(det, dev) as K:
        c0 = K.unordered_launches()
        runs = []
        for _ in range(2 if det else 1):
            xq, ls = K.vq_gather_loss(xt, et, it, mt)
            runs.append([xq, ls] + [K.vq_backward(gt, xt, et, it, mt, c) for c in coefs]
                        + [K.vq_embed(et, it, torch.float32), K.vq_embed(et, it, dtype)])
        torch.cuda.synchronize()
        if det:
            for a, b in zip(*runs):
                assert torch.equal(a, b), f"{what}: deterministic mode: identical launches differ"
            assert K.unordered_launches() == c0, f"{what}: deterministic mode took an unordered path"
        elif rows > 4:
            assert K.unordered_launches() > c0, f"{what}: several workgroups with the mode off were not counted as unordered"
    xq, ls, dx0, dx1, emb32, embt = runs[0]
    want = M.straight_through_bf16(x, e, idx) if dtype == torch.bfloat16 else M.straight_through_f32(x, e, idx)
    _bits_equal(_host(xq), want, "x_q " + what)
    _bits_equal(_host(emb32), M.gather(e, idx), "embed fp32 " + what)
    _bits_equal(_host(embt), _rnd(M.gather(e, idx), dtype), "embed in the row type " + what)
    r = M.row_sqerr(x, e, idx)
    weight = r if mask is None else np.abs(mask.astype(np.float64)) * r
    ref = M.loss_sum(x, e, idx, mask)
    form = (math.ceil(d / 64) + 8) * float(weight.sum())
    _pin("loss", _host(ls).reshape(()), ref, form + rows * 2.0 ** -29 * abs(ref), what="loss " + what)
    if ceiling:
        assert FP32_K["loss"] * U * form <= CEIL_LOSS * abs(ref), f"loss {what}: the bound is above rtol {CEIL_LOSS}"
    diff = np.abs(x.astype(np.float64) - M.gather(e, idx))
    m64 = np.ones((rows, 1)) if mask is None else mask.astype(np.float64)[:, None]
    for c, dx in zip(COEFS, (dx0, dx1)):
        c32 = float(np.float32(c))
        dref = M.backward(g, x, e, idx, mask, c32)
        _pin("dx", _host(dx), dref, 2 * abs(c32) * m64 * diff + np.abs(dref), dtype, what=f"dx coef {c} " + what)
    return runs[0]


GATHER_ROWS = [1, 3, 4, 5, 16384, 16385, 2 * 16384 + 3]
GATHER_D = [1, 63, 64, 65, 256, 264]


@MODES
@pytest.mark.parametrize("masked", [False, True], ids=["no-mask", "mask"])
@DTYPES
@pytest.mark.parametrize("rows", GATHER_ROWS)
def test_gather_rows(dev, rows, dtype, masked, det):
    """1 / 3 (dead waves), 4 (exactly one workgroup), 5 (a second one), 16 384 (4096 workgroups, every wave one row), 16 385 and
    2 x 16 384 + 3 (the grid-stride trip); D 65 (a second lane trip of one element), K 5"""
    _gather_case(dev, rows, 65, 5, dtype, masked, det, ceiling=not masked)


@MODES
@pytest.mark.parametrize("masked", [False, True], ids=["no-mask", "mask"])
@DTYPES
@pytest.mark.parametrize("d", GATHER_D)
def test_gather_widths(dev, d, dtype, masked, det):
    """D below, at and above the wave width, the product's 256 and 264 = 4 trips + 8; 37 rows (ten workgroups, three dead waves),
    K 1024 with idx hitting rows 0 and 1023"""
    _gather_case(dev, 37, d, 1024, dtype, masked, det, ceiling=not masked)


def _fallback_launch(dev):
    """deterministic mode without scratch at 4099 rows: the loss sum runs as ONE workgroup.  -> (x_q, loss sum) on the device"""
    K = _k()
    from dynamicvectorquantization_amd._lib import check
    x, g, e, idx, mask = _gather_operands(4099, 65, 5, False, True)
    try:
        check(K.lib().dvq_set_workspace(None, 0), "dvq_set_workspace")
        K._workspace.clear()
        K.set_deterministic(True)
        c0 = K.unordered_launches()
        xq, ls = K.vq_gather_loss(_dev(x, dev), _dev(e, dev), _dev(idx, dev), _dev(mask, dev))
        torch.cuda.synchronize()
        assert K.unordered_launches() == c0, "deterministic mode without scratch took an unordered path"
    finally:
        K.set_deterministic(False)
        K.ensure_workspace(dev)
    return xq, ls


def _fingerprint(xq, ls):
    return f"{_host(ls).reshape(-1).view(np.uint64)[0]:016x} {zlib.crc32(_host(xq).tobytes()):08x}"


def test_gather_one_workgroup_fallback(dev):
    """the mode on with dvq_set_workspace(None, 0) at 4099 rows: values within the same bounds, two launches of this process
    bit-identical, and two fresh processes give the same bits as this one"""
    x, g, e, idx, mask = _gather_operands(4099, 65, 5, False, True)
    a, b = _fallback_launch(dev), _fallback_launch(dev)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), "one-workgroup fallback: identical launches differ"
    _bits_equal(_host(a[0]), M.straight_through_f32(x, e, idx), "x_q one-workgroup fallback")
    ref = M.loss_sum(x, e, idx, mask)
    form = (math.ceil(65 / 64) + 8) * float((np.abs(mask.astype(np.float64)) * M.row_sqerr(x, e, idx)).sum())
    _pin("loss", _host(a[1]).reshape(()), ref, form + 4099 * 2.0 ** -29 * abs(ref), what="loss one-workgroup fallback")
    kids = [subprocess.Popen([sys.executable, os.path.abspath(__file__), "fallback"], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                             text=True) for _ in range(2)]
    outs = [p.communicate(timeout=240) for p in kids]
    for p, (so, se) in zip(kids, outs):
        assert p.returncode == 0, f"fresh process failed ({p.returncode}):\n{se[-2000:]}"
    prints = [[l for l in so.splitlines() if l.startswith("FALLBACK ")][-1][9:] for so, _ in outs]
    assert prints[0] == prints[1] == _fingerprint(*a), f"fresh processes: {prints}, this process: {_fingerprint(*a)}"
    # the workspace is back: the split form runs again and meets the same bound
    _gather_case(dev, 4099, 65, 5, torch.float32, True, True)


def test_embed_multi_dimensional_idx_and_out_view(dev):
    """idx [2, 3, 5] -> [2, 3, 5, D]; out= a view into a larger buffer, as the restart-row path passes it (VQEmbedding._exchange_buffers)"""
    K = _k()
    rs = np.random.RandomState(61)
    k, d = 9, 72
    e = rs.standard_normal((k, d)).astype(np.float32)
    idx = rs.randint(0, k, (2, 3, 5)).astype(np.int64)
    et, it = _dev(e, dev), _dev(idx, dev)
    for dtype in (torch.float32, torch.bfloat16):
        got = K.vq_embed(et, it, dtype)
        assert tuple(got.shape) == (2, 3, 5, d) and got.dtype == dtype
        _bits_equal(_host(got), _rnd(M.gather(e, idx), dtype), f"embed {dtype}")
    flat = torch.full((k * (d + 1) + k * d + 4,), -3.0, device=dev)
    view = flat[k * (d + 1):k * (d + 1) + k * d].view(k, d)
    perm = rs.permutation(30)[:k].astype(np.int64)
    src = rs.standard_normal((30, d)).astype(np.float32)
    got = K.vq_embed(_dev(src, dev), _dev(perm, dev), out=view)
    torch.cuda.synchronize()
    _bits_equal(_host(view), M.gather(src, perm), "embed into a view")
    assert got.data_ptr() == view.data_ptr()
    assert bool((flat[:k * (d + 1)] == -3.0).all()) and bool((flat[-4:] == -3.0).all()), "embed wrote outside its view"


# ==== vq_ema_apply =======================================================================================================================
def _apply(dev, n0, s0, stats, restart, decay, eps, pad):
    """-> (n_ema, s_ema, weight [K + 1, D]) after dvq_vq_ema_apply on copies"""
    K = _k()
    k, d = s0.shape
    nt, st = _dev(n0.astype(np.float32), dev), _dev(s0.astype(np.float32), dev)
    wt = torch.cat([torch.full((k, d), float("nan"), device=dev), _dev(pad.astype(np.float32), dev)[None]]).contiguous()
    K.vq_ema_apply(_dev(stats.astype(np.float32), dev), None if restart is None else _dev(restart.astype(np.float32), dev),
                   decay, eps, nt, st, wt)
    torch.cuda.synchronize()
    return _host(nt), _host(st), _host(wt)


def _apply_check(dev, n0, s0, cnt, sums, restart, decay, eps, what, ceiling=None, off_edge=True):
    """n_ema and s_ema against ema_update; weight against ema_normalize of the kernel's OWN n_ema / s_ema (the normalise kernel reads
    those).  Forms: n_ema |n0 decay| + |cnt (1 - decay)|; s_ema |s0 decay| + |sum (1 - decay)|; weight |w| (3 + ceil(K / 256) + 9):
    eps joins n_k, K eps joins n_tot, the product, two divisions, and n_tot itself -- ceil(K / 256) adds per thread, eight tree levels"""
    k, d = s0.shape
    pad = np.arange(d) * 0.5 - 1.0
    stats = np.concatenate([sums, cnt[:, None]], axis=1)
    n1, s1, w1 = _apply(dev, n0, s0, stats, restart, decay, eps, pad)
    rn, rs_, dead = M.ema_update(n0, s0, cnt, sums, decay, restart)
    live = ~dead
    nn = np.asarray(n0, dtype=np.float64) * decay + cnt * (1.0 - decay)
    f_n = np.abs(n0 * decay) + np.abs(cnt * (1.0 - decay))
    if restart is not None and off_edge:                       # every count is farther from the dead-code rule's 1 than its bound
        finite = np.isfinite(nn)
        assert bool((np.abs(nn[finite] - 1.0) > FP32_K["n_ema"] * U * f_n[finite]).all()), f"{what}: a count within its bound of the dead-code rule"
    assert bool((n1[dead] == 1.0).all()), f"{what}: a dead code's count is not exactly 1"
    _pin("n_ema", n1[live], rn[live], f_n[live], ceiling=ceiling, what=what)
    if restart is not None:
        _bits_equal(s1[dead], restart[dead].astype(np.float32), f"{what}: a dead code's row is not its restart row")
    _pin("s_ema", s1[live], rs_[live], (np.abs(s0 * decay) + np.abs(sums * (1.0 - decay)))[live], ceiling=ceiling, what=what)
    _bits_equal(w1[k], pad.astype(np.float32), f"{what}: the padding row")
    wref = M.ema_normalize(n1, s1, eps)
    _pin("weight", w1[:k], wref, np.abs(wref) * (3 + math.ceil(k / 256) + 9), ceiling=ceiling, what=what)
    return n1, s1, w1, dead


def test_ema_apply_dead_code_boundary(dev):
    """decay 0.5 makes n' exact: (n0, cnt) = (2, 0) -> 1 lives, (1.5, 0) -> 0.75 dies, (0, 2) -> 1 lives, (0, 0) dies, NaN dies.
    Dead: n_ema = 1 exactly, s_ema = the restart row bit for bit.  The restart rows of the live codes are NaN: nothing reads them"""
    rs = np.random.RandomState(71)
    d = 5
    n0 = np.array([2.0, 1.5, 0.0, 0.0, np.nan])
    cnt = np.array([0.0, 0.0, 2.0, 0.0, 0.0])
    s0, sums = rs.standard_normal((5, d)), rs.standard_normal((5, d)) * (cnt[:, None] > 0)
    restart = rs.standard_normal((5, d))
    restart[[0, 2]] = np.nan
    for det in (False, True):
        with _mode(det):
            n1, s1, w1, dead = _apply_check(dev, n0, s0, cnt, sums, restart, 0.5, EPS, f"boundary det {int(det)}", off_edge=False)
        assert list(dead) == [False, True, False, True, True]
        assert list(n1) == [1.0, 1.0, 1.0, 1.0, 1.0]
        # no restart rows: nothing dies below 1; every weight is finite (n_tot > 0)
        with _mode(det):
            n2, s2, w2, dead2 = _apply_check(dev, n0[:4], s0[:4], cnt[:4], sums[:4], None, 0.5, EPS, f"boundary, no restart rows, det {int(det)}")
        assert not dead2.any() and list(n2) == [1.0, 0.75, 1.0, 0.0]
    # the one exception: every count zero -> n_tot = 0, the normaliser is 0 eps / (K eps) = 0 and the reference divides by it too
    zeros = np.zeros(4)
    stats = np.zeros((4, d + 1))
    _, s3, w3 = _apply(dev, zeros, s0[:4], stats, None, 0.5, EPS, np.zeros(d))
    with np.errstate(all="ignore"):
        wref = M.ema_normalize(zeros, s3, EPS)
    assert not np.isfinite(wref).any() and not np.isfinite(w3[:4]).any()
    assert np.array_equal(np.isnan(w3[:4]), np.isnan(wref)) and np.array_equal(np.sign(w3[:4][~np.isnan(wref)]), np.sign(wref[~np.isnan(wref)]))


def _apply_operands(k, d, seed):
    rs = np.random.RandomState(seed)
    n0 = np.where(rs.rand(k) < 0.2, 0.0, 10.0 ** rs.uniform(-2, 4, k)).astype(np.float32).astype(np.float64)       # 0 .. 1e4
    cnt = np.where(rs.rand(k) < 0.3, 0.0, rs.randint(0, 400, k)).astype(np.float64)
    if k > 1:
        n0[0], cnt[0], n0[1] = 0.0, 0.0, 1e4                                                 # one code that dies, one that lives
    nn = n0 * DECAY + cnt * (1.0 - DECAY)
    n0 = np.where(np.abs(nn - 1.0) < 1e-2, n0 + 1.0, n0)                                    # keep every count away from the rule's edge
    s0 = (rs.standard_normal((k, d)) * n0[:, None]).astype(np.float32).astype(np.float64)
    sums = (rs.standard_normal((k, d)) * np.sqrt(cnt)[:, None]).astype(np.float32).astype(np.float64)
    restart = rs.standard_normal((k, d)).astype(np.float32).astype(np.float64)
    return n0, s0, cnt, sums, restart


APPLY_SIZES = [(7, 1), (7, 255), (7, 256), (7, 257), (7, 1024), (1, 5), (255, 5), (256, 5), (257, 5), (1027, 5)]


@MODES
@pytest.mark.parametrize("with_restart", [True, False], ids=["restart-rows", "no-restart-rows"])
@pytest.mark.parametrize("k,d", APPLY_SIZES, ids=[f"K{k}-D{d}" for k, d in APPLY_SIZES])
def test_ema_apply_sizes(dev, k, d, with_restart, det):
    """the D-strided loops at their tails (D 1, 255, 256, 257, 1024) and the K-strided sum with its tree (K 1, 255, 256, 257, 1027);
    decay 0.99, eps 1e-5, n0 from 0 to 1e4"""
    n0, s0, cnt, sums, restart = _apply_operands(k, d, 300 + 13 * k + d)
    if not with_restart and not (n0 * DECAY + cnt * (1.0 - DECAY)).sum() > 0:
        n0 = n0 + 3.0                                                                        # (K = 1: keep n_tot > 0 -- the exception has its own case)
    with _mode(det):
        n1, s1, w1, dead = _apply_check(dev, n0, s0, cnt, sums, restart if with_restart else None, DECAY, EPS,
                                        f"K {k} D {d} restart {int(with_restart)} det {int(det)}", ceiling=CEIL_EMA)
    if k > 1:
        assert bool(dead[0]) == with_restart and not dead[1]
    assert np.isfinite(w1).all()


@MODES
@pytest.mark.parametrize("k", [257, 1027])
def test_ema_apply_small_total(dev, k, det):
    """n_tot enters the weight only through n_tot / (n_tot + K eps): with counts of 1e2 and more a wrong sum over the codes moves no
    weight by its bound.  Here every count lies in 1e-4 .. 1e-2 (no rows, no restart rows), n_tot is of the order of K eps, and the
    strided sum above 256 codes shows in every weight"""
    rs = np.random.RandomState(500 + k)
    d = 5
    n0 = (10.0 ** rs.uniform(-4, -2, k)).astype(np.float32).astype(np.float64)
    s0 = (rs.standard_normal((k, d)) * n0[:, None]).astype(np.float32).astype(np.float64)
    assert 0.1 < n0.sum() / (k * EPS) < 1000
    with _mode(det):
        _apply_check(dev, n0, s0, np.zeros(k), np.zeros((k, d)), None, DECAY, EPS, f"small total K {k} det {int(det)}")


# ==== vq_distances =======================================================================================================================
_BASE = (17, 65, 33)
DIST_CASES = sorted(set([(n, _BASE[1], _BASE[2]) for n in (1, 15, 16, 17, 29)] + [(_BASE[0], k, _BASE[2]) for k in (1, 63, 64, 65, 130)]
                        + [(_BASE[0], _BASE[1], d) for d in (1, 31, 32, 33, 64, 256)]
                        + [(n, k, d) for n in (1, 29) for k in (1, 130) for d in (1, 256)]))


@MODES
@DTYPES
@pytest.mark.parametrize("n,k,d", DIST_CASES, ids=[f"N{n}-K{k}-D{d}" for n, k, d in DIST_CASES])
def test_distances_tile_edges(dev, n, k, d, dtype, det):
    """64 codes x 16 rows x 32 dims per stage: one axis at a time around (17, 65, 33), and the corners.  Form: (D / 32 + 3)
    (|x|^2 + |e|^2 + 2 sum |x e|) -- the three fused sums of D terms and the two final operations, first order"""
    rs = np.random.RandomState(1000 * n + 10 * k + d)
    x = _rnd(1.5 * rs.standard_normal((n, d)) + 0.25, dtype)
    e = (1.5 * rs.standard_normal((k, d))).astype(np.float32)
    with _mode(det) as K:
        out = torch.full((n, k), float("nan"), device=dev)
        got = K.vq_distances(_dev(x, dev, dtype), _dev(e, dev), out=out)
        torch.cuda.synchronize()
    x64, e64 = x.astype(np.float64), e.astype(np.float64)
    form = (d / 32 + 3) * ((x64 ** 2).sum(1)[:, None] + (e64 ** 2).sum(1)[None] + 2 * np.abs(x64) @ np.abs(e64).T)
    _pin("distances", _host(got), M.distances(x, e), form, ceiling=CEIL_DIST, what=f"N {n} K {k} D {d} {_tag(dtype, det)}")


# ==== dual_merge, dual_merge_bwd: bit-exact ============================================================================================
def _raw(t):
    """device tensor -> numpy of its bits (bf16 as int16): selections are compared without arithmetic"""
    t = t.detach().contiguous()
    return (t.view(torch.int16) if t.dtype == torch.bfloat16 else t).cpu().numpy()


def _grain_map(kind, shape, rs):
    if kind == "coarse":
        return np.zeros(shape, dtype=np.int64)
    if kind == "fine":
        return rs.choice([1, 2, -1], shape).astype(np.int64)
    return rs.choice([0, 1, 2, -1], shape, p=[0.5, 0.2, 0.15, 0.15]).astype(np.int64)       # 2 and -1 count as fine


@MODES
@DTYPES
@pytest.mark.parametrize("kind", ["coarse", "fine", "mixed"])
@pytest.mark.parametrize("shape", [(2, 3, 5, 8), (1, 1, 1, 264), (2, 4, 4, 256)], ids=lambda s: "x".join(map(str, s)))
def test_dual_merge_exact(dev, shape, kind, dtype, det):
    """out = the selected source bit for bit, mask exactly 1 / 0.25; gf = g on fine cells and 0 on coarse ones; gc = the four gradients
    added from zero in the kernel's order in fp32, one rounding to the type, 0 on fine cells"""
    b, h, w, c = shape
    rs = np.random.RandomState(b + 3 * h + 5 * w + c + len(kind))
    hf, hc = _rnd(rs.standard_normal((b, 2 * h, 2 * w, c)), dtype), _rnd(rs.standard_normal((b, h, w, c)), dtype)
    g = _rnd(rs.standard_normal((b, 2 * h, 2 * w, c)), dtype)
    grain = _grain_map(kind, (b, h, w), rs)
    hft, hct, gt, grt = _dev(hf, dev, dtype), _dev(hc, dev, dtype), _dev(g, dev, dtype), _dev(grain, dev)
    with _mode(det) as K:
        out, mask = K.dual_merge(hft, hct, grt)
        gf, gc = K.dual_merge_bwd(gt, grt)
        torch.cuda.synchronize()
    want, wmask = M.dual_merge(_raw(hft), _raw(hct), grain)
    _bits_equal(_raw(out), want, "dual merge")
    _bits_equal(_host(mask), wmask.astype(np.float32), "dual merge mask")
    fine = np.repeat(np.repeat(grain != 0, 2, 1), 2, 2)[..., None]
    _bits_equal(_host(gf), np.where(fine, g, np.float32(0)), "dual merge: fine gradient")
    _bits_equal(_host(gc), _rnd(M.dual_merge_bwd_coarse_f32(g, grain), dtype), "dual merge: coarse gradient")
    _pin("merge_grad", _host(gc), M.dual_merge_bwd(g, grain)[1], 4 * M.dual_merge_bwd(np.abs(g), grain)[1], dtype, what="dual merge coarse vs fp64")


def test_dual_merge_second_grid_trip(dev):
    """(2, 32, 33, 2048) bf16: 2 162 688 vectors against the forward's cap of 8192 x 256 = 2 097 152 -- the grid-stride trip the product
    starts with one image more than 64 per GPU.  (The backward has a quarter of the vectors: no second trip at this shape)"""
    K = _k()
    b, h, w, c = 2, 32, 33, 2048
    assert b * 4 * h * w * c // 8 == 2162688 > 8192 * 256
    gen = torch.Generator(device="cpu").manual_seed(5)
    hf = torch.randn((b, 2 * h, 2 * w, c), generator=gen).to(torch.bfloat16).view(torch.int16)       # compared as bits: a selection, no arithmetic
    hc = torch.randn((b, h, w, c), generator=gen).to(torch.bfloat16).view(torch.int16)
    grain = _grain_map("mixed", (b, h, w), np.random.RandomState(6))
    out, mask = K.dual_merge(hf.to(dev).view(torch.bfloat16), hc.to(dev).view(torch.bfloat16), _dev(grain, dev))
    torch.cuda.synchronize()
    want, wmask = M.dual_merge(hf.numpy(), hc.numpy(), grain)
    _bits_equal(_raw(out), want, "dual merge, second trip")
    _bits_equal(_host(mask), wmask.astype(np.float32), "dual merge mask, second trip")


def test_dual_merge_rejects_c12(dev):
    K = _k()
    hf, hc = torch.zeros(1, 2, 2, 12, device=dev), torch.zeros(1, 1, 1, 12, device=dev)
    grain = torch.zeros(1, 1, 1, dtype=torch.int64, device=dev)
    with pytest.raises(_err_type()):
        K.dual_merge(hf, hc, grain)
    with pytest.raises(_err_type()):
        K.dual_merge_bwd(hf, grain)


# ==== grain_merge, grain_merge_bwd ======================================================================================================
@MODES
@DTYPES
@pytest.mark.parametrize("cells", [(2, 1, 1), (2, 3, 5)], ids=["1x1", "3x5"])
@pytest.mark.parametrize("c", [8, 64, 520])
@pytest.mark.parametrize("s", [2, 3])
def test_grain_merge_edges(dev, s, c, cells, dtype, det):
    """S 2 / 3; C 8 (one lane of the backward), 64 (8 lanes), 520 (65 vectors: a second lane-loop trip); N 2; a mixed map and every
    all-one-level map; scale absent / present, dscale wanted / not.
    Forward without scale and the mask: bit for bit.  With scale: |got - ref| <= 2^-24 |ref| (one fp32 product) + the bf16 term.
    Gradients: unselected levels exactly 0; selected |got - ref| <= (terms + 1) 2^-24 sum|g| |s| (terms = 1 / 4 / 16 added in fp32, then the
    product) + the bf16 term.  dscale: (8 + ceil(C / 8 / 64) + 6) sum |acc h| -- a lane's fused adds and the wave's tree, measured K"""
    n, hc, wc = cells
    f = 1 << (s - 1)
    rs = np.random.RandomState(97 * s + c + hc)
    heads = [_rnd(rs.standard_normal((n, hc << l, wc << l, c)), dtype) for l in range(s)]
    g = _rnd(rs.standard_normal((n, hc * f, wc * f, c)), dtype)
    scale = (rs.rand(n, hc, wc) + 0.5).astype(np.float32)
    ht, gt, sct = [_dev(h, dev, dtype) for h in heads], _dev(g, dev, dtype), _dev(scale, dev)
    maps = [("mixed", rs.randint(0, s, (n, hc, wc)).astype(np.int64))] + [(f"all-{l}", np.full((n, hc, wc), l, dtype=np.int64)) for l in range(s)]
    for name, idx in maps:
        it = _dev(idx, dev)
        for use_scale, want_ds in ((False, False), (True, True), (True, False), (False, True)):
            what = f"S {s} C {c} cells {hc}x{wc} {name} scale {int(use_scale)} dscale {int(want_ds)} {_tag(dtype, det)}"
            sc_np, sc_t = (scale, sct) if use_scale else (None, None)
            with _mode(det) as K:
                out, mask = K.grain_merge(ht, it, sc_t)
                dh, ds = K.grain_merge_bwd(gt, ht, it, sc_t, want_dscale=want_ds)
                torch.cuda.synchronize()
            ref, rmask = M.grain_merge(heads, idx, sc_np)
            _bits_equal(_host(mask), rmask.astype(np.float32), "mask " + what)
            if use_scale:
                _pin("merge", _host(out), ref, np.abs(ref), dtype, what="merged " + what)
            else:
                _bits_equal(_host(out), ref.astype(np.float32), "merged " + what)
            rdh, rds, mag = M.grain_merge_bwd(g, heads, idx, sc_np)
            adh, _, _ = M.grain_merge_bwd(np.abs(g), heads, idx, None if sc_np is None else np.abs(sc_np))
            lvl_of = [np.repeat(np.repeat(idx == l, 1 << l, 1), 1 << l, 2) for l in range(s)]
            for l in range(s):
                got = _host(dh[l])
                assert not bool(got[~lvl_of[l]].any()), f"gradient of unselected level {l} is not zero: {what}"
                terms = 4 ** (s - 1 - l)
                _pin("merge_grad", got, rdh[l], (terms + 1) * adh[l], dtype, what=f"d head {l} " + what)
            if want_ds:
                _pin("dscale", _host(ds), rds, (8 + math.ceil(c / 8 / 64) + 6) * mag, what="dscale " + what)
            else:
                assert ds is None


# ==== avgpool_slice, avgpool_slice_bwd ==================================================================================================
@MODES
@DTYPES
@pytest.mark.parametrize("c", [8, 72])
@pytest.mark.parametrize("k", [1, 2, 4])
def test_avgpool_slice_edges(dev, k, c, dtype, det):
    """k x k means into the channel slice [coff, coff + C) of rows ldy wide, coff = 16 > 0 and ldy = coff + C + 24; the columns outside
    the slice keep their sentinel.  |got - ref| <= (k^2 + 1) 2^-24 mean|x| (k^2 adds, the product with 1 / k^2) + the bf16 term.
    Backward: dy / k^2 is exact in fp32 (k^2 a power of two) -- 2^-24 |ref| covers it -- + the bf16 term"""
    n, h, w, coff = 2, 3, 5, 16
    ldy = coff + c + 24
    rs = np.random.RandomState(10 * k + c)
    x = _rnd(rs.standard_normal((n, h * k, w * k, c)) + 0.5, dtype)
    with _mode(det) as K:
        y = torch.full((n, h, w, ldy), -7.0, device=dev, dtype=dtype)
        K.avgpool_slice(_dev(x, dev, dtype), k, y, coff)
        dx = K.avgpool_slice_bwd(y, coff, c, k)
        torch.cuda.synchronize()
    yh = _host(y)
    assert bool((yh[..., :coff] == -7.0).all()) and bool((yh[..., coff + c:] == -7.0).all()), "the pool wrote outside its slice"
    what = f"k {k} C {c} {_tag(dtype, det)}"
    _pin("pool", yh[..., coff:coff + c], M.avgpool(x, k), (k * k + 1) * M.avgpool(np.abs(x), k), dtype, what="pool " + what)
    ref = M.avgpool_bwd(yh[..., coff:coff + c], k)
    assert tuple(dx.shape) == (n, h * k, w * k, c)
    _pin("pool", _host(dx), ref, np.abs(ref), dtype, what="pool backward " + what)


def test_avgpool_slice_rejections(dev):
    """k = 3; coff % 8 != 0; a slice that ends past the row: DvqError, nothing written"""
    K = _k()
    x = torch.ones(1, 12, 12, 8, device=dev)
    y = torch.full((1, 4, 4, 32), -7.0, device=dev)
    for k, coff in ((3, 8), (2, 4), (2, 32)):
        yy = y if k == 3 else torch.full((1, 6, 6, 32), -7.0, device=dev)
        with pytest.raises(_err_type()):
            K.avgpool_slice(x, k, yy, coff)
        with pytest.raises(_err_type()):
            K.avgpool_slice_bwd(yy, coff, 8, k)
        torch.cuda.synchronize()
        assert bool((yy == -7.0).all())


# ==== the layers ===========================================================================================================================
def _quantiser(dev, k, d, e, n0, s0, perm):
    from dynamicvectorquantization_amd.quantize import VectorQuantize2
    vq = VectorQuantize2(codebook_size=k, codebook_dim=d).to(dev).train()
    cb = vq.codebook
    with torch.no_grad():
        cb.weight.copy_(_dev(np.concatenate([e, np.full((1, d), 0.125, dtype=np.float32)]), dev))
        cb.embed_ema.copy_(_dev(s0, dev))
        cb.cluster_size_ema.copy_(_dev(n0, dev))
    cb.restart_perm = _dev(perm, dev)
    return vq


@DTYPES
def test_layer_vector_quantize2_training(dev, dtype):
    """VectorQuantize2.fwd / bwd with a tape, training mode: N 1100 = 2 x 22 x 25 rows (a second slice of 76 rows), K 70, D 72 (the
    generic search), injected restart_perm, mask from {1, 1/4, 1/16, 0}.  idx against oracle.vq.argmin_exact; everything behind the
    search against vq_math on that idx; the backward runs after the EMA rewrite and must use the codebook from before it"""
    from dynamicvectorquantization_amd import runtime as rt
    from dynamicvectorquantization_amd.layers import Tape
    from oracle import vq as ovq
    b, hh, ww, k, d, beta = 2, 22, 25, 70, 72, 0.25
    n = b * hh * ww
    rs = np.random.RandomState(83)
    e = (0.8 * rs.standard_normal((k, d))).astype(np.float32)
    x = _rnd(rs.standard_normal((n, d)), dtype)
    x[:40] = _rnd(e[rs.randint(0, 5, 40)] + 0.05 * rs.standard_normal((40, d)), dtype)         # some rows sit close to codes 0 .. 4
    g = _rnd(rs.standard_normal((n, d)), dtype)
    mask = rs.choice(MASK_VALUES, n).astype(np.float32)
    n0 = rs.choice([0.0, 0.5, 5.0, 50.0], k).astype(np.float32)
    s0 = (e * n0[:, None]).astype(np.float32)
    perm = rs.permutation(n).astype(np.int64)
    idx = ovq.argmin_exact(x, e)
    sums, cnt = M.code_sums(x, idx, k)
    sabs, _ = M.code_sums(np.abs(x), idx, k)
    nn = n0.astype(np.float64) * DECAY + cnt * (1.0 - DECAY)
    assert bool((np.abs(nn - 1.0) > 1e-3).all()) and 0 < int((nn < 1).sum()) < k
    with rt.compute_dtype_ctx(dtype):
        vq = _quantiser(dev, k, d, e, n0, s0, perm)
        tape = Tape()
        xq, loss, got_idx = vq.fwd(_dev(x, dev, dtype).view(b, hh, ww, d), _dev(mask, dev).view(b, hh, ww), tape)
        g_loss = torch.tensor(3.0, device=dev)
        dx = vq.bwd(_dev(g, dev, dtype).view(b, hh, ww, d), g_loss, tape)
        torch.cuda.synchronize()
    what = f"VectorQuantize2 {_tag(dtype, False)}"
    assert np.array_equal(_host(got_idx).reshape(-1), idx), f"{what}: idx differs from the exact argmin"
    want = M.straight_through_bf16(x, e, idx) if dtype == torch.bfloat16 else M.straight_through_f32(x, e, idx)
    _bits_equal(_host(xq).reshape(n, d), want, "x_q " + what)
    # loss = loss_sum (1 + beta) / numel in fp64, one rounding to fp32
    r = M.row_sqerr(x, e, idx)
    lref = M.vq_loss(x, e, idx, mask, beta)
    lform = (math.ceil(d / 64) + 8) * float((mask * r).sum()) * (1 + beta) / (n * d) + abs(lref)
    _pin("loss", _host(loss).reshape(()), lref, lform, what="loss " + what)
    # EMA buffers: the statistics' bound carried through the blend
    cb = vq.codebook
    restart = M.gather(x, perm[:k])
    rn, rs_, dead = M.ema_update(n0, s0, cnt, sums, DECAY, restart)
    slices = np.zeros(k)
    for s in range(0, n, EMA_SLICE):
        slices[np.unique(idx[s:s + EMA_SLICE])] += 1
    n1, s1, w1 = _host(cb.cluster_size_ema), _host(cb.embed_ema), _host(cb.weight)
    live = ~dead
    assert bool((n1[dead] == 1.0).all())
    _pin("n_ema", n1[live], rn[live], (np.abs(n0 * DECAY) + np.abs(cnt * (1.0 - DECAY)))[live], what=what)
    _bits_equal(s1[dead], restart[dead].astype(np.float32), f"{what}: dead rows against x[restart_perm]")
    # (the statistics' own derived bound enters with the constant 1: divided here by the K that _pin multiplies the form with)
    f_s = np.abs(s0 * DECAY) + np.abs(sums * (1.0 - DECAY)) + (cnt + slices)[:, None] * sabs * (1.0 - DECAY) / FP32_K["s_ema"]
    _pin("s_ema", s1[live], rs_[live], f_s[live], what=what)
    wref = M.ema_normalize(n1, s1, EPS)
    _pin("weight", w1[:k], wref, np.abs(wref) * (3 + math.ceil(k / 256) + 9), what=what)
    assert bool((w1[k] == 0.125).all()), "the padding row moved"
    assert float(np.abs(w1[:k] - e).max()) > 1e-3, "the codebook was not rewritten: the backward check below would prove nothing"
    # dx = g + coef mask (x - e_old); coef = g_loss 2 beta / numel formed on the host side in fp32: one more rounding than the kernel's form
    coef = float(np.float32(3.0) * np.float32(2.0 * beta / (n * d)))
    dref = M.backward(g, x, e, idx, mask, coef)
    diff = np.abs(x.astype(np.float64) - M.gather(e, idx))
    _pin("dx", _host(dx).reshape(n, d), dref, 3 * abs(coef) * mask.astype(np.float64)[:, None] * diff + np.abs(dref), dtype, what="dx " + what)


def test_layer_restart_with_fewer_rows_than_codes(dev):
    """N 20 < K 64: the candidate rows are the batch tiled 4 times plus U[0, 1) 0.01 / sqrt(D) noise.  Every code is dead (counts 0), so
    every row of embed_ema is a restart row: it lies in [src, src + 0.01 / sqrt(D)) of its tiled source row -- as stored, i.e. after
    the one fp32 rounding of src + noise"""
    from dynamicvectorquantization_amd import runtime as rt
    n, k, d = 20, 64, 72
    rs = np.random.RandomState(89)
    e = rs.standard_normal((k, d)).astype(np.float32)
    x = rs.standard_normal((n, d)).astype(np.float32)
    perm = rs.permutation(4 * n).astype(np.int64)
    with rt.compute_dtype_ctx(torch.float32):
        vq = _quantiser(dev, k, d, e, np.zeros(k, dtype=np.float32), np.zeros((k, d), dtype=np.float32), perm)
        emb, idx = vq.codebook(_dev(x, dev).view(1, n, d))
        torch.cuda.synchronize()
    _bits_equal(_host(emb).reshape(n, d), M.gather(e, _host(idx).reshape(-1)), "embeds come from the codebook before the rewrite")
    assert bool((_host(vq.codebook.cluster_size_ema) == 1.0).all())
    src = x[perm[:k] % n].astype(np.float64)
    off = _host(vq.codebook.embed_ema).astype(np.float64) - src
    width = 0.01 / math.sqrt(d)
    assert bool((off >= 0).all()) and bool((off < width + U * (np.abs(src) + width)).all()), (off.min(), off.max(), width)
    assert off.max() > 0.5 * width and off.min() < 0.5 * width and len(np.unique(off)) > off.size // 2, "the noise is not spread over its interval"


def test_layer_dual_grain_encoder_merge_call(dev, monkeypatch):
    """DualGrainEncoder.fwd with a fixed-entropy grain map: what it returns is vq_math's dual merge of the two heads it handed over
    (fine head first), and the mask goes with it"""
    from dynamicvectorquantization_amd import runtime as rt
    from dynamicvectorquantization_amd import synth
    from dynamicvectorquantization_amd.config import instantiate_from_config, stage1_config
    K = _k()
    seen = {}
    real = K.dual_merge

    def spy(h_fine, h_coarse, grain):
        seen.update(hf=h_fine, hc=h_coarse, grain=grain)
        return real(h_fine, h_coarse, grain)

    with rt.compute_dtype_ctx(torch.bfloat16):
        torch.manual_seed(0)
        model = instantiate_from_config(stage1_config(objective="ae", geometry=synth.DQVAE_GEOM["small"]).model).to(dev).eval()
        img = torch.from_numpy(synth.half_flat_images(1, 64, seed=5)).to(dev)
        enc = model.encoder
        with torch.no_grad():
            assert not enc.feature_routed
            hc = 64 // 16
            grain = _dev(_grain_map("mixed", (1, hc, hc), np.random.RandomState(7)), dev)
            monkeypatch.setattr(K, "dual_merge", spy)
            merged, mask, routing = enc.fwd(img, grain, None)
            torch.cuda.synchronize()
    assert routing is None and seen["hf"].shape[1] == 2 * seen["hc"].shape[1] == 2 * hc
    want, wmask = M.dual_merge(_raw(seen["hf"]), _raw(seen["hc"]), _host(seen["grain"]))
    _bits_equal(_raw(merged), want, "DualGrainEncoder: merged")
    _bits_equal(_host(mask), wmask.astype(np.float32), "DualGrainEncoder: mask")
    assert len(np.unique(_host(mask))) == 2


if __name__ == "__main__" and sys.argv[1:] == ["fallback"]:
    # a fresh process of test_gather_one_workgroup_fallback: the same launch, its bits on one line
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    print("FALLBACK " + _fingerprint(*_fallback_launch(torch.device("cuda:0"))))
