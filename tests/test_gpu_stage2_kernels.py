"""The stage-2 transformer's row and pointwise kernels (csrc/transformer.hip; dvq_softmax_rows, dvq_softmax_rows_bwd and dvq_transpose of
csrc/misc.hip), each called through kernels.py at the smallest shapes that reach every edge of its dispatch, compared PER ELEMENT with
the fp64 references of tests/stage2_math.py.  docs/design/25-stage2-kernel-pins.md has the edge -> case table and the tolerances.

Operands are drawn from a seeded RandomState and rounded to the tensor type before the reference sees them.  Bounds:
  bf16 outputs   |got - ref| <= 2^-8 |ref| + the fp32 term: one correctly rounded bf16 store on top of the fp32 arithmetic (derived);
  fp32 results   |got - ref| <= K 2^-24 (first-order magnitude of the operation's terms) + 2^-126.  The form is stated at each family,
                 K is FP32_K[family]: four times the largest error of the fp32 kernel against the fp64 reference over the family's
                 cases (FP32_MEASURED, one run on an MI355X).  2^-126 is the smallest normal fp32: below it a result has no relative
                 precision to hold.
Where deterministic mode changes the path both modes run and meet the same bound.
Not coverable here: element indices >= 2^32 of the dropout hash (a tensor of more than 8 GB) and the grid-stride trips of the
one-wave-per-row kernels beyond 262 144 rows."""
import contextlib

import numpy as np
import pytest
import torch

import stage2_math as M

pytestmark = pytest.mark.gpu

U = 2.0 ** -24            # fp32 unit roundoff
BF = 2.0 ** -8            # bf16 unit roundoff (round to nearest even, 8 significant bits)
TINY = 2.0 ** -126        # smallest normal fp32

# largest (error - 2^-126) / (2^-24 x form) of the fp32 kernels over each family's cases, both modes, one run on an MI355X
FP32_MEASURED = {
    "ln_fwd_stats": 1.741, "ln_fwd_y": 1.307, "ln_bwd_dx": 1.433, "ln_bwd_param": 0.4398, "gelu": 0.8375, "gelu_bwd": 2.197,
    "softmax": 2.25, "softmax_bwd": 1.784, "softmax_causal": 2.104, "ce_loss": 0.6758, "ce_grad": 1.952, "embed_scatter": 1.0,
}
# chosen: four times the measurement (different summation orders between modes and launches)
FP32_K = {family: 4.0 * worst for family, worst in FP32_MEASURED.items()}
# what the suite already accepts for the same kind of value: the chosen bound of the regular cases stays below it
CEIL_POINTWISE = 1e-5     # O(1) pointwise values (test_nonlinearity_standalone)
CEIL_NORM = 2e-4          # normalisation outputs (test_groupnorm)

DTYPES = pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
MODES = pytest.mark.parametrize("det", [False, True], ids=["mode-off", "deterministic"])


def _k():
    from dynamicvectorquantization_amd import kernels as K
    return K


@contextlib.contextmanager
def _mode(det):
    K = _k()
    try:
        K.set_deterministic(det)
        yield K
    finally:
        K.set_deterministic(False)


def _rnd(a, dtype):
    """fp64 draw -> the value the tensor type holds, as fp32"""
    a = np.asarray(a, dtype=np.float64).astype(np.float32)
    return M.bf16_round(a) if dtype == torch.bfloat16 else a


def _dev(a, dev, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return t if dtype is None else t.to(dtype)


def _np(t):
    return t.detach().double().cpu().numpy()


def _pin(family, got, ref, form, dtype=torch.float32, ceiling=None, regular=None, what=""):
    """per element: |got - ref| <= FP32_K[family] 2^-24 form + 2^-126 (+ 2^-8 |ref| for a bf16 tensor).  Prints the fp32 ratio.
    ceiling: what the chosen fp32 term may reach on the elements marked `regular` (default: all)"""
    got, ref = _np(got) if torch.is_tensor(got) else np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    unit = U * np.broadcast_to(np.asarray(form, np.float64), ref.shape)
    assert np.isfinite(got).all(), f"{family} {what}: non-finite output"
    err = np.abs(got - ref)
    if dtype == torch.float32:
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(unit > 0, np.maximum(err - TINY, 0.0) / unit, np.where(err > TINY, np.inf, 0.0))
        print(f"PIN {family} {float(ratio.max()):.4g} {what}")
    k = FP32_K[family]
    bound = k * unit + TINY + (BF * np.abs(ref) if dtype == torch.bfloat16 else 0.0)
    bad = err > bound
    if bad.any():
        w = np.unravel_index(np.argmax(err - bound), err.shape)
        raise AssertionError(f"{family} {what}: {int(bad.sum())} of {bad.size} elements out of bound; worst at {w}: got {got[w]!r} "
                             f"ref {ref[w]!r} err {err[w]:.3e} bound {bound[w]:.3e}")
    if ceiling is not None:
        sel = unit if regular is None else unit[np.broadcast_to(regular, unit.shape)]
        top = k * float(sel.max()) if sel.size else 0.0
        assert top <= ceiling, f"{family} {what}: chosen fp32 bound {top:.3e} above {ceiling}"
    return bound


# ---- LayerNorm forward --------------------------------------------------------------------------------------------------------------
LN_FWD = [(r, c, ms) for (r, c) in ((1, 8), (7, 72), (5, 512), (6, 520), (9, 1024), (3, 4096)) for ms in (0, 2)] + [(9, 1024, 8)]


@DTYPES
@pytest.mark.parametrize("rows,c,musig", LN_FWD, ids=[f"{r}x{c}-mu{m}sigma" for r, c, m in LN_FWD])
def test_layernorm_fwd(dev, rows, c, musig, dtype):
    """x = sigma N(0,1) + mu.  The kernel forms var = E[x^2] - mean^2 in fp32, so the relative error of rstd, and through it the error
    of y, carries the factor kappa = E[x^2] / (var + eps):
      mean: 2^-24 mean|x|      rstd: 2^-24 rstd kappa      y: 2^-24 (kappa (|xhat| + 1) |gamma| + |y|).
    mu / sigma = 8 (kappa 65) cannot meet the bound of the centred cases by design; it is kept with the same kappa-scaled form."""
    K = _k()
    rs = np.random.RandomState(1000 * musig + rows + c)
    sigma = 1.5
    x = _rnd(sigma * rs.standard_normal((rows, c)) + musig * sigma, dtype)
    gamma = (1 + 0.2 * rs.standard_normal(c)).astype(np.float32)
    beta = (0.2 * rs.standard_normal(c)).astype(np.float32)
    y_ref, mean_ref, rstd_ref = M.layernorm_fwd(x, gamma, beta, 1e-5)
    y, mr = K.layernorm_fwd(_dev(x, dev, dtype), _dev(gamma, dev), _dev(beta, dev), 1e-5)
    x64 = x.astype(np.float64)
    kappa = (x64 ** 2).mean(1) * rstd_ref ** 2
    xh = (x64 - mean_ref[:, None]) * rstd_ref[:, None]
    tag = f"{rows}x{c} mu/sigma {musig}"
    _pin("ln_fwd_stats", mr[:, 0], mean_ref, np.abs(x64).mean(1), what="mean " + tag)
    _pin("ln_fwd_stats", mr[:, 1], rstd_ref, rstd_ref * kappa, what="rstd " + tag)
    _pin("ln_fwd_y", y, y_ref, kappa[:, None] * (np.abs(xh) + 1) * np.abs(gamma) + np.abs(y_ref), dtype,
         ceiling=CEIL_NORM if musig <= 2 else None, what=tag)


# ---- LayerNorm backward -------------------------------------------------------------------------------------------------------------
LN_BWD = [(5, c) for c in (8, 72, 512, 520, 1024, 1032, 2048, 2056, 4096)] + [(r, c) for r in (37, 261, 4099) for c in (72, 1024)]


def _ln_bwd_inputs(rows, c, dtype, dev, seed):
    K = _k()
    rs = np.random.RandomState(seed)
    x = _rnd(1.5 * rs.standard_normal((rows, c)) + 0.5, dtype)
    dy = _rnd(rs.standard_normal((rows, c)), dtype)
    dres = _rnd(rs.standard_normal((rows, c)), dtype)
    gamma = (1 + 0.2 * rs.standard_normal(c)).astype(np.float32)
    dg0, db0 = rs.standard_normal(c).astype(np.float32), rs.standard_normal(c).astype(np.float32)
    xt, gt = _dev(x, dev, dtype), _dev(gamma, dev)
    _, mr = K.layernorm_fwd(xt, gt, torch.zeros(c, device=dev), 1e-5)
    return x, dy, dres, gamma, dg0, db0, xt, gt, mr


@MODES
@DTYPES
@pytest.mark.parametrize("rows,c", LN_BWD, ids=[f"{r}x{c}" for r, c in LN_BWD])
def test_layernorm_bwd(dev, rows, c, dtype, det):
    """mean / rstd are the forward kernel's own (the reference takes the same fp32 values).  dgamma / dbeta start non-zero: the entry adds.
      dx:     2^-24 (rstd (|g| + mean|g| + (|xhat| + (|x| + |mean|) rstd) mean|g xhat|) + |dres| + |dx|),  g = dy gamma
      dgamma: m 2^-24 (sum over rows |dy| (|x| + |mean|) rstd + |start|),  dbeta: m 2^-24 (sum |dy| + |start|),  m = rows + 1 addends."""
    x, dy, dres, gamma, dg0, db0, xt, gt, mr = _ln_bwd_inputs(rows, c, dtype, dev, 31 * rows + c)
    mean, rstd = _np(mr[:, 0]), _np(mr[:, 1])
    x64, dy64 = x.astype(np.float64), dy.astype(np.float64)
    xh = (x64 - mean[:, None]) * rstd[:, None]
    g = dy64 * gamma
    spread = (np.abs(x64) + np.abs(mean)[:, None]) * rstd[:, None]
    dyt = _dev(dy, dev, dtype)
    for res in (None, dres):
        dx_ref, dg_ref, db_ref = M.layernorm_bwd(x, dy, gamma, 1e-5, dres=res, mean=mean, rstd=rstd)
        dg, db = _dev(dg0, dev), _dev(db0, dev)
        with _mode(det) as K:
            dx = K.layernorm_bwd(xt, dyt, mr, gt, dg, db, dres=None if res is None else _dev(res, dev, dtype))
        tag = f"{rows}x{c} dres {'absent' if res is None else 'present'} det {det}"
        form = rstd[:, None] * (np.abs(g) + np.abs(g).mean(1, keepdims=True) + (np.abs(xh) + spread) * np.abs(g * xh).mean(1, keepdims=True))
        form = form + np.abs(dx_ref) + (0.0 if res is None else np.abs(res.astype(np.float64)))
        _pin("ln_bwd_dx", dx, dx_ref, form, dtype, ceiling=CEIL_NORM, what=tag)
        m = rows + 1
        _pin("ln_bwd_param", dg, dg_ref + dg0, m * ((np.abs(dy64) * spread).sum(0) + np.abs(dg0)), what="dgamma " + tag)
        _pin("ln_bwd_param", db, db_ref + db0, m * (np.abs(dy64).sum(0) + np.abs(db0)), what="dbeta " + tag)


@DTYPES
@pytest.mark.parametrize("rows,c", [(333, 1032), (5, 72)], ids=["333x1032", "5x72"])
def test_layernorm_bwd_dropout_output(dev, rows, c, dtype):
    """the second output is dropout(dx, p, seed) bit for bit, and its zeros are the host mirror's"""
    K = _k()
    x, dy, dres, gamma, dg0, db0, xt, gt, mr = _ln_bwd_inputs(rows, c, dtype, dev, rows + c)
    p, seed = 0.1, (1 << 33) + 5
    dx, dxd = K.layernorm_bwd(xt, _dev(dy, dev, dtype), mr, gt, _dev(dg0, dev), _dev(db0, dev), dres=_dev(dres, dev, dtype), drop=(p, seed))
    assert torch.equal(dxd, K.dropout(dx, p, seed))
    keep = M.dropout_keep(rows * c, p, seed).reshape(rows, c)
    assert np.array_equal(_np(dxd) != 0, keep & (_np(dx) != 0))
    assert 0 < int((~keep).sum()) < rows * c


# ---- GELU ---------------------------------------------------------------------------------------------------------------------------
def _gelu_forms(x):
    phi = np.exp(-0.5 * x * x) / np.sqrt(2 * np.pi)
    return np.abs(x) + np.abs(M.gelu(x)), 1 + np.abs(x) * phi * (1 + 0.5 * x * x)


def test_gelu_bf16_all_patterns(dev):
    """every bf16 bit pattern in one launch.  forward: 2^-24 (|x| + |gelu x|) (erff is absolute at 1, multiplied by x);
    backward: 2^-24 |dy| (1 + |x| phi(x) (1 + x^2 / 2)) (__expf is relative in its argument).  NaN goes through as NaN, +-inf faults nothing."""
    K = _k()
    bits = torch.arange(65536, dtype=torch.int32, device=dev).to(torch.int16)
    xt = bits.view(torch.bfloat16)
    x = _np(xt)
    fin, nan = np.isfinite(x), np.isnan(x)
    assert fin.sum() == 65536 - 256 and nan.sum() == 254
    xf = x[fin]
    f_fwd, f_bwd = _gelu_forms(xf)
    y = _np(K.gelu(xt))
    assert np.isnan(y[nan]).all()
    _pin("gelu", y[fin], M.gelu(xf), f_fwd, torch.bfloat16, what="bf16 patterns")
    rs = np.random.RandomState(5)
    for name, dy in (("ones", np.ones(65536, np.float32)), ("random", _rnd(rs.standard_normal(65536), torch.bfloat16))):
        d = _np(K.gelu_bwd(xt, _dev(dy, dev, torch.bfloat16)))
        assert np.isnan(d[nan]).all()
        dyf = dy.astype(np.float64)[fin]
        _pin("gelu_bwd", d[fin], dyf * M.gelu_grad(xf), np.abs(dyf) * f_bwd, torch.bfloat16, what="bf16 patterns dy " + name)
    torch.cuda.synchronize()


@pytest.mark.parametrize("n", [8, 8 * 257])
def test_gelu_fp32(dev, n):
    K = _k()
    rs = np.random.RandomState(n)
    x = rs.uniform(-12, 12, n)
    special = [0.0, 1e-30, -1e-4, 5.5, -5.5, 9.0, -9.0, 40.0] if n == 8 else [0.0, 1e-30, -1e-30, 1e-4, -1e-4, 5.5, -5.5, 9.0, -9.0, 40.0, -40.0]
    x[:len(special)] = special
    x = _rnd(x, torch.float32)
    dy = _rnd(rs.standard_normal(n), torch.float32)
    x64, dy64 = x.astype(np.float64), dy.astype(np.float64)
    f_fwd, f_bwd = _gelu_forms(x64)
    xt = _dev(x, dev)
    y = K.gelu(xt)
    _pin("gelu", y, M.gelu(x64), f_fwd, ceiling=CEIL_POINTWISE, regular=np.abs(x64) <= 2, what=f"fp32 n {n}")
    d = K.gelu_bwd(xt, _dev(dy, dev))
    _pin("gelu_bwd", d, dy64 * M.gelu_grad(x64), np.abs(dy64) * f_bwd, what=f"fp32 n {n}")
    d1 = K.gelu_bwd(xt, torch.ones(n, device=dev))
    _pin("gelu_bwd", d1, M.gelu_grad(x64), f_bwd, ceiling=CEIL_POINTWISE, what=f"fp32 n {n} dy 1")


# ---- softmax over rows and its backward ---------------------------------------------------------------------------------------------
def _softmax_form(z, p, vis=None):
    """2^-24 p (1 + |z| + max|z|): the scaled score and the row maximum are rounded to fp32 before the difference, __expf is
    relative in its argument"""
    az = np.abs(z) if vis is None else np.where(vis, np.abs(z), 0.0)
    return p * (1 + az + az.max(axis=1, keepdims=True))


@DTYPES
@pytest.mark.parametrize("scale", [1 / 8.0, -1 / 0.37], ids=["scale0.125", "scale-2.7"])
@pytest.mark.parametrize("rows", [1, 7])
@pytest.mark.parametrize("length", [1, 63, 64, 65, 200, 1024])
def test_softmax_rows(dev, length, rows, scale, dtype):
    """rows = 7: row 3 holds +-80 / |scale| (only the subtraction of the maximum keeps it finite).
    backward: 2^-24 |scale| p (|dp| + 2 sum|p dp|), p and dp as the tensors hold them."""
    K = _k()
    rs = np.random.RandomState(length * 16 + rows)
    s = 2 * rs.standard_normal((rows, length))
    if rows == 7:
        s[3] = np.where(rs.rand(length) < 0.5, -1.0, 1.0) * 80 / abs(scale)
    s = _rnd(s, dtype)
    z = s.astype(np.float64) * np.float64(np.float32(scale))
    p_ref = M.softmax_rows(s, np.float32(scale))
    tag = f"{rows}x{length} scale {scale:.3g}"
    p = K.softmax_rows(_dev(s, dev, dtype), rows, length, scale)
    bound = _pin("softmax", p, p_ref, _softmax_form(z, p_ref), dtype, ceiling=CEIL_POINTWISE, regular=np.abs(z).max(1, keepdims=True) <= 8,
                 what=tag)
    assert (np.abs(_np(p).sum(1) - 1.0) <= bound.sum(1)).all()
    p_in, dp = _rnd(p_ref, dtype), _rnd(rs.standard_normal((rows, length)), dtype)
    ds = K.softmax_rows_bwd(_dev(p_in, dev, dtype), _dev(dp, dev, dtype), rows, length, scale)
    p64, dp64 = p_in.astype(np.float64), dp.astype(np.float64)
    form = abs(scale) * p64 * (np.abs(dp64) + 2 * np.abs(p64 * dp64).sum(1, keepdims=True))
    _pin("softmax_bwd", ds, M.softmax_rows_bwd(p_in, dp, np.float32(scale)), form, dtype, ceiling=CEIL_POINTWISE, what=tag)


CAUSAL = [(2, 1, 1, 0), (260, 65, 65, 0), (600, 200, 200, 0), (12, 70, 3, 67), (4, 10, 4, 9)]


@DTYPES
@pytest.mark.parametrize("rows,length,tq,offset", CAUSAL, ids=[f"{r}x{l}-tq{t}-off{o}" for r, l, t, o in CAUSAL])
def test_softmax_causal(dev, rows, length, tq, offset, dtype):
    """in place; row r sees columns <= r % Tq + offset.  (12, 70, 3, 67) is the K/V-cache form, (4, 10, 4, 9) has the visible range
    clipped to L.  Masked columns are exactly 0."""
    K = _k()
    scale = 1 / 8.0
    rs = np.random.RandomState(rows + length)
    s = _rnd(3 * rs.standard_normal((rows, length)), dtype)
    vis = np.arange(length)[None, :] < M.causal_valid(rows, length, tq, offset)[:, None]
    p_ref = M.softmax_causal(s, tq, offset, scale)
    st = _dev(s, dev, dtype)
    out = K.softmax_causal_(st, rows, length, tq, offset, scale)
    assert out.data_ptr() == st.data_ptr()
    got = _np(st)
    assert (got[~vis] == 0.0).all()
    bound = _pin("softmax_causal", st, p_ref, _softmax_form(s.astype(np.float64) * scale, p_ref, vis), dtype, ceiling=CEIL_POINTWISE,
                 what=f"{rows}x{length} tq {tq} off {offset}")
    assert (np.abs(got.sum(1) - 1.0) <= bound.sum(1)).all()


# ---- transpose ----------------------------------------------------------------------------------------------------------------------
TRANSPOSE = [(torch.bfloat16, r, c) for r, c in ((64, 64), (72, 8), (643, 64), (65, 72), (8, 1024), (5, 7))] + \
            [(torch.float32, r, c) for r, c in ((33, 31), (32, 32), (643, 64))]


@pytest.mark.parametrize("dtype,r,c", TRANSPOSE, ids=[f"{'bf16' if d == torch.bfloat16 else 'fp32'}-{r}x{c}" for d, r, c in TRANSPOSE])
def test_transpose(dev, dtype, r, c):
    """bf16 with C % 8 == 0: the 64 x 64 kernel with 16-byte stores (R % 8 == 0) or 2-byte stores; everything else: the 32 x 32 kernel"""
    K = _k()
    rs = np.random.RandomState(r + c)
    x = _dev(_rnd(rs.standard_normal((3, r, c)), dtype), dev, dtype)
    assert torch.equal(K.transpose(x, 3, r, c).view(3, c, r), x.transpose(1, 2).contiguous())


def test_transpose_unaligned_view(dev):
    """a contiguous bf16 view that starts one element into its buffer is 2-byte aligned: the generic kernel takes it"""
    K = _k()
    rs = np.random.RandomState(2)
    buf = _dev(_rnd(rs.standard_normal(3 * 64 * 64 + 8), torch.bfloat16), dev, torch.bfloat16)
    x = buf[1:1 + 3 * 64 * 64].view(3, 64, 64)
    assert x.is_contiguous() and x.data_ptr() % 16 == 2
    assert torch.equal(K.transpose(x, 3, 64, 64).view(3, 64, 64), x.transpose(1, 2).contiguous())


# ---- embedding gather ---------------------------------------------------------------------------------------------------------------
@DTYPES
@pytest.mark.parametrize("shared", [False, True], ids=["index-per-batch", "shared-index-row"])
@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("c", [8, 72])
@pytest.mark.parametrize("t0", [0, 4])
def test_embed_gather(dev, t0, c, accumulate, shared, dtype):
    K = _k()
    b, ln, ttot, v = 3, 5, 9, 11
    rs = np.random.RandomState(100 * t0 + c + accumulate)
    idx = torch.from_numpy(rs.randint(0, v, (ln,) if shared else (b, ln)).astype(np.int64))
    table = torch.from_numpy(rs.standard_normal((v, c)).astype(np.float32))
    out0 = torch.from_numpy(_rnd(rs.standard_normal((b, ttot, c)), dtype)).to(dtype)
    rows = table[idx.expand(b, ln) if shared else idx]
    ref = out0.clone()
    ref[:, t0:t0 + ln] = (out0[:, t0:t0 + ln].float() + rows).to(dtype) if accumulate else rows.to(dtype)
    out = out0.to(dev)
    K.embed_gather(idx.to(dev), table.to(dev), out, t0, accumulate, bstride=0 if shared else None)
    assert torch.equal(out.cpu(), ref)                      # rows outside [t0, t0 + len) included: unchanged bit for bit


# ---- embedding scatter-add ----------------------------------------------------------------------------------------------------------
def _scatter_case(name, rs):
    """-> idx, B, Ttot, t0, C, V, padding row"""
    if name == "split-16rows":                              # 7 splits of 115 tokens
        return rs.randint(0, 16, (8, 100)), 8, 100, 0, 64, 16, 3
    if name == "full-window":                               # one split, windows [0, 1024) [1024, 2048) [2048, 2600); the second is ALL row 5
        flat = np.where(rs.rand(2600) < 0.505, 5, rs.randint(0, 600, 2600))
        flat[1024:2048] = 5
        assert abs((flat == 5).mean() - 0.7) < 0.03
        return flat.reshape(2, 1300), 2, 1300, 0, 8, 600, 7
    if name == "every-thread-owns":                         # C / 8 = 256
        return rs.randint(0, 600, (1, 130)), 1, 130, 0, 2048, 600, 7
    if name == "t0-shared-row":
        return rs.randint(0, 16, (5,)), 3, 12, 3, 64, 16, 3
    if name == "atomics-wide":                              # C > 2048
        return rs.randint(0, 16, (2, 50)), 2, 50, 0, 2056, 16, 3
    if name == "atomics-tall":                              # V > 65535
        return rs.randint(0, 65536, (2, 50)), 2, 50, 0, 8, 65536, 3
    raise KeyError(name)


SCATTER = ["split-16rows", "full-window", "every-thread-owns", "t0-shared-row", "atomics-wide", "atomics-tall"]


@MODES
@DTYPES
@pytest.mark.parametrize("name", SCATTER)
def test_embed_scatter_add(dev, name, dtype, det):
    """per element: hits(v) 2^-24 (sum|terms| + |start|) -- a row without hits and the padding row keep their bits.  The per-token
    atomics beyond V 65535 / C 2048 have no ordered form: deterministic mode rejects them on the host, ahead of any launch."""
    from dynamicvectorquantization_amd import _lib
    rs = np.random.RandomState(SCATTER.index(name) + 40)
    idx, b, ttot, t0, c, v, pad = _scatter_case(name, rs)
    idx = idx.astype(np.int64)
    idx.reshape(-1)[1] = pad
    if name != "full-window":
        idx.reshape(-1)[2] = 5
    shared = idx.ndim == 1
    dout = _rnd(rs.standard_normal((b, ttot, c)), dtype)
    start = rs.standard_normal((v, c)).astype(np.float32)
    dtable = _dev(start, dev)
    it, dt_ = _dev(idx, dev), _dev(dout, dev, dtype)
    with _mode(det) as K:
        if det and name.startswith("atomics"):
            with pytest.raises(_lib.DvqError):
                K.embed_scatter_add(it, dt_, dtable, t0, padding_idx=pad, bstride=0 if shared else None)
            assert torch.equal(dtable.cpu(), torch.from_numpy(start))
            return
        K.embed_scatter_add(it, dt_, dtable, t0, padding_idx=pad, bstride=0 if shared else None)
    ref = M.embed_scatter_add(idx, dout, start, t0, padding_idx=pad)
    mag = M.embed_scatter_add(idx, np.abs(dout), np.abs(start), t0, padding_idx=pad)
    hits = M.embed_hits(idx, b, v, pad)
    assert hits[5] > 0 and hits[pad] == 0
    if name == "full-window":
        assert hits[5] >= 1024
    _pin("embed_scatter", dtable, ref, hits[:, None] * mag, what=f"{name} det {det}")
    assert torch.equal(dtable[pad].cpu(), torch.from_numpy(start[pad]))


# ---- cross entropy ------------------------------------------------------------------------------------------------------------------
CE_SHAPES = [(5, 5), (67, 67), (67, 72), (1024, 1024), (1027, 1027), (1027, 1032), (2026, 2032), (2048, 2048), (2049, 2056)]
CE = [(v, ldl, rows) for v, ldl in CE_SHAPES for rows in (1, 7)] + [(1027, 1032, 4101)]
IGNORE = -100
GSCALE = 0.37


def ce_inputs(rs, rows, v, ldl, dtype, every=3):
    """padding columns hold +30; rows 2, 5, 8, ... are ignored; targets include V - 1 and 0; row 3 holds one +60 among -60s"""
    logits = np.full((rows, ldl), 30.0)
    logits[:, :v] = 3 * rs.standard_normal((rows, v))
    target = rs.randint(0, v, rows).astype(np.int64)
    target[0] = v - 1
    if rows > 3:
        target[1] = 0
        logits[3, :v] = -60.0
        logits[3, v // 2] = 60.0
    target[every - 1::every] = IGNORE
    return _rnd(logits, dtype), target


def ce_loss_check(logits, v, target, start, loss_sum, count, what):
    """loss sum: 2^-24 (n_live + 1) (sum over live rows (|max| + |log sum| + |logit[target]|) + |start|)   (n_live + 1 addends)"""
    x = logits.astype(np.float64)
    rows = x.shape[0]
    loss_ref, cnt_ref, _ = M.cross_entropy(x, v, target, IGNORE)
    live = target != IGNORE
    z = x[:, :v]
    mx = z.max(1)
    lse = np.log(np.exp(z - mx[:, None]).sum(1))
    tg = np.where(live, target, 0)
    terms = (np.abs(mx) + np.abs(lse) + np.abs(z[np.arange(rows), tg]))[live].sum()
    assert float(count) == start[1] + cnt_ref
    _pin("ce_loss", loss_sum.reshape(()), np.float64(loss_ref + start[0]), (cnt_ref + 1) * (terms + abs(start[0])), what=what)


def ce_grad_check(logits, v, target, gscale, dl, dtype, what, ignore_index=IGNORE):
    """dlogits: 2^-24 |gscale| (p (1 + |x| + |max|) + onehot); exact zeros in ignored rows and padding columns; live rows sum to 0
    (test_gpu_reproducible.py applies the same check to the ordered form)"""
    x = logits.astype(np.float64)
    rows = x.shape[0]
    _, _, d_ref = M.cross_entropy(x, v, target, ignore_index, gscale)
    live = target != ignore_index
    z = x[:, :v]
    mx = z.max(1, keepdims=True)
    got = _np(dl)
    assert (got[:, v:] == 0.0).all(), "padding columns of dlogits are not zero"
    assert (got[~live] == 0.0).all(), "ignored rows of dlogits are not zero"
    p = np.exp(z - mx) / np.exp(z - mx).sum(1, keepdims=True)
    onehot = np.zeros_like(z)
    onehot[np.arange(rows)[live], target[live]] = 1.0
    form = np.zeros_like(x)
    form[:, :v] = abs(gscale) * (p * (1 + np.abs(z) + np.abs(mx)) + onehot) * live[:, None]
    bound = _pin("ce_grad", dl, d_ref, form, dtype, ceiling=CEIL_POINTWISE, regular=(np.abs(z).max(1) <= 8)[:, None], what=what)
    assert (np.abs(got[:, :v].sum(1)) <= bound[:, :v].sum(1))[live].all(), "a live row of dlogits does not sum to 0"


@MODES
@DTYPES
@pytest.mark.parametrize("v,ldl,rows", CE, ids=[f"V{v}-ld{l}-{r}rows" for v, l, r in CE])
def test_cross_entropy(dev, v, ldl, rows, dtype, det):
    """ldl % 8 != 0 or ldl > 2048: the scalar kernel; ldl <= 1024: two vectors per lane; ldl <= 2048: four.  4101 rows: 1024 workgroups,
    the first wave makes a second grid-stride trip.  loss_sum and count start non-zero: the entry adds."""
    rs = np.random.RandomState(v + ldl + rows)
    logits, target = ce_inputs(rs, rows, v, ldl, dtype)
    start = (1.5, 3.0)
    ls, cnt = torch.full((1,), start[0], device=dev), torch.full((1,), start[1], device=dev)
    with _mode(det) as K:
        dl = K.cross_entropy(_dev(logits, dev, dtype), v, _dev(target, dev), IGNORE, ls, cnt, gscale=torch.full((1,), GSCALE, device=dev),
                             want_grad=True)
    what = f"V {v} ldl {ldl} rows {rows} det {det}"
    ce_loss_check(logits, v, target, start, ls, cnt, what)
    ce_grad_check(logits, v, target, np.float64(np.float32(GSCALE)), dl, dtype, what)


@MODES
@DTYPES
@pytest.mark.parametrize("v,ldl", [(1027, 1027), (1027, 1032)], ids=["scalar-rows", "vector-rows"])
def test_cross_entropy_every_row_ignored(dev, v, ldl, dtype, det):
    rs = np.random.RandomState(v + ldl)
    logits, _ = ce_inputs(rs, 7, v, ldl, dtype)
    ls, cnt = torch.zeros(1, device=dev), torch.zeros(1, device=dev)
    with _mode(det) as K:
        dl = K.cross_entropy(_dev(logits, dev, dtype), v, torch.full((7,), IGNORE, dtype=torch.int64, device=dev), IGNORE, ls, cnt,
                             gscale=torch.full((1,), GSCALE, device=dev), want_grad=True)
    assert float(ls) == 0.0 and float(cnt) == 0.0 and not bool(dl.any())


# ---- dropout ------------------------------------------------------------------------------------------------------------------------
@DTYPES
@pytest.mark.parametrize("n", [8, 8 * 257, 8 * 70001])
def test_dropout_mask_contract(dev, n, dtype):
    """the zero pattern is the host mirror of dvq_hash32 / dvq_dropout_seed bit for bit (seed 2^33 + 5 uses the seed's high word); kept
    values are the fp32 product x (1 / (1 - p)) rounded to the tensor type; dropout_add is add(x, dropout(a)); p = 0 is a plain add.
    Element indices >= 2^32 would need a tensor of more than 8 GB: the high-word term of the index is only covered by the host mirror's
    own CPU test."""
    K = _k()
    rs = np.random.RandomState(n % 1000)
    a = _rnd(rs.standard_normal(n) + np.where(rs.rand(n) < 0.5, 0.25, -0.25), dtype)         # (no zeros: a zero output is a dropped one)
    assert (a != 0).all()
    x = _rnd(rs.standard_normal(n), dtype)
    at, xt = _dev(a, dev, dtype), _dev(x, dev, dtype)
    for p in (0.0, 0.1, 0.5, 0.999):
        for seed in (17, 987654321, (1 << 33) + 5):
            keep = M.dropout_keep(n, p, seed)
            y = K.dropout(at, p, seed)
            prod = a * M.dropout_scale(p)
            want = np.where(keep, M.bf16_round(prod) if dtype == torch.bfloat16 else prod, np.float32(0))
            got = y.float().cpu().numpy()
            assert np.array_equal(got != 0, keep), f"mask differs from the host mirror: n {n} p {p} seed {seed}"
            assert np.array_equal(got, want), f"kept values: n {n} p {p} seed {seed}"
            ya = K.dropout_add(xt, at, p, seed)
            assert torch.equal(ya, K.add(xt, y)), f"dropout_add: n {n} p {p} seed {seed}"
            if p == 0.0:
                assert keep.all() and torch.equal(ya, xt + at)


# ---- host-side argument rejections (DVQ_REQUIRE, ahead of any launch) ---------------------------------------------------------------
def test_argument_rejections(dev):
    from dynamicvectorquantization_amd import _lib
    K = _k()

    def z(*shape):
        return torch.zeros(*shape, device=dev)

    with pytest.raises(_lib.DvqError):
        K.layernorm_bwd(z(5, 4104), z(5, 4104), z(5, 2), z(4104), z(4104), z(4104))
    with pytest.raises(_lib.DvqError):
        K.gelu(z(12))
    with pytest.raises(_lib.DvqError):
        K.layernorm_fwd(z(2, 12), z(12), z(12))
    with pytest.raises(_lib.DvqError):
        K.embed_gather(torch.zeros(3, 5, dtype=torch.int64, device=dev), z(11, 8), z(3, 9, 8), 5, 0)
    torch.cuda.synchronize()
