"""The stage-1 normalisation family (csrc/groupnorm.hip: dvq_gn_stats, dvq_gn_scale_shift, dvq_gn_apply, dvq_gn_bwd_reduce with its
finalize kernel, dvq_gn_bwd_dx), called through kernels.gn_stats / gn_forward / gn_scale_shift / gn_backward as Normalize, BatchNorm2d
and ActNorm call them, at the smallest shapes that reach every edge of the dispatch, compared PER ELEMENT with the fp64 references of
tests/stage1_norm_math.py.  docs/design/26-groupnorm-kernel-pins.md has the edge -> case table and the tolerances.

Operands are drawn from a seeded RandomState and rounded to the tensor type before the reference sees them.  Bounds:
  stats          |got - ref| <= m 2^-24 (sum|x|, sum x^2), m = ceil(pixels per workgroup / pixel rows per pass): a thread adds m values
                 of a channel in fp32 before anything is combined in fp64 (derived; the bound of test_gn_stats_kernel_ordered);
  mean, rstd     dmean = dS / cnt + 2^-24 |mean|,  drstd / rstd = (dQ / cnt + 2 |mean| dS / cnt) / (2 (var + eps)) + 2^-24 (derived from
                 the statistics bound: one fp32 rounding on top of fp64 arithmetic);
  bf16 outputs   |got - ref| <= 2^-8 |ref| + the fp32 term: one correctly rounded bf16 store on top of the fp32 arithmetic (derived);
  fp32 results   |got - ref| <= K 2^-24 (first-order magnitude of the operation's terms) + 2^-126.  The form is stated at each family
                 (_forward_forms, _backward_forms), K is FP32_K[family]: four times the largest error of the fp32 kernel against the
                 fp64 reference over every case of this file, both modes (FP32_MEASURED, one run on an MI355X).  y and the {scale, shift}
                 table carry dmean and drstd with sqrt(m) in place of m (_stat_bounds); the backward takes the forward's fp32 mean_rstd.
Where deterministic mode changes the path both modes run and meet the same bound, and two launches with the mode on are bit-identical.
Not coverable here: N > 65535 beyond its rejection; the halo convolution's statistics epilogue and GroupNorm prologue keep their tests."""
import contextlib
import functools
import math

import numpy as np
import pytest
import torch

import stage1_norm_math as M

pytestmark = pytest.mark.gpu

U = 2.0 ** -24            # fp32 unit roundoff
BF = 2.0 ** -8            # bf16 unit roundoff (round to nearest even, 8 significant bits)
TINY = 2.0 ** -126        # smallest normal fp32

# largest (error - 2^-126) / (2^-24 x form) of the fp32 kernels over every case of this file, both modes, one run on an MI355X
FP32_MEASURED = {"scale_shift": 0.654, "y": 0.8937, "dx": 0.4904, "dparam": 0.2898}
# chosen: four times the measurement (other summation orders between modes and launches)
FP32_K = {family: 4.0 * worst for family, worst in FP32_MEASURED.items()}
# derived bounds carry no constant
FP32_K.update(stats=1.0, mean=1.0, rstd=1.0)
CEIL_NORM = 2e-4          # test_groupnorm accepts rtol = atol = 2e-4 on y and dx: the chosen fp32 bound of the regular cases stays below it

ACTS = (M.ACT_NONE, M.ACT_SWISH, M.ACT_LRELU)
ACT_NAME = {M.ACT_NONE: "none", M.ACT_SWISH: "swish", M.ACT_LRELU: "lrelu"}
ACT_SLOPE = {M.ACT_NONE: 1.0, M.ACT_SWISH: 1.1, M.ACT_LRELU: 1.0}          # sup |act'|  (swish: 1.0998)
ACT_CURV = {M.ACT_NONE: 0.0, M.ACT_SWISH: 0.5, M.ACT_LRELU: 0.0}           # sup |act''| away from LeakyReLU's kink
EPS = float(np.float32(1e-6))

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


def _no_workspace(monkeypatch):
    """no registered scratch: deterministic launches run unsplit (as test_gpu_reproducible.py does it)"""
    K = _k()
    from dynamicvectorquantization_amd._lib import check
    check(K.lib().dvq_set_workspace(None, 0), "dvq_set_workspace")
    K._workspace.clear()
    monkeypatch.setattr(K, "ensure_workspace", lambda device: None)


def _rnd(a, dtype):
    """fp64 draw -> the value the tensor type holds, as an fp32 tensor"""
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
    return M.bf16_round(t) if dtype == torch.bfloat16 else t


def _pin(family, got, ref, form, dtype=torch.float32, extra=None, ceiling=None, what=""):
    """per element: |got - ref| <= FP32_K[family] 2^-24 form + 2^-126 (+ extra) (+ 2^-8 |ref| for a bf16 tensor).  Prints the fp32
    ratio.  extra: an absolute allowance (LeakyReLU's kink).  ceiling: the chosen fp32 term stays below ceiling (1 + |ref|), which is
    what assert_allclose(rtol = atol = ceiling) accepts"""
    ref = ref.double()
    got = got.detach().to(ref.device).double().reshape(ref.shape)
    unit = U * torch.broadcast_to(torch.as_tensor(form, dtype=torch.float64, device=ref.device), ref.shape)
    assert bool(torch.isfinite(got).all()), f"{family} {what}: non-finite output"
    err = (got - ref).abs()
    slack = TINY if extra is None else TINY + torch.broadcast_to(extra, ref.shape)
    if dtype == torch.float32:
        over = (err - slack).clamp(min=0.0)
        ratio = torch.where(unit > 0, over / unit.clamp(min=1e-300), torch.where(over > 0, torch.full_like(over, math.inf), torch.zeros_like(over)))
        print(f"PIN {family} {float(ratio.max()):.4g} {what}")
    k = FP32_K[family]
    bound = k * unit + slack
    if dtype == torch.bfloat16:
        bound = bound + BF * ref.abs()
    bad = err > bound
    if bool(bad.any()):
        w = int(torch.argmax((err - bound).reshape(-1)))
        idx = tuple(int(i) for i in np.unravel_index(w, tuple(err.shape)))
        raise AssertionError(f"{family} {what}: {int(bad.sum())} of {bad.numel()} elements out of bound; worst at {idx}: "
                             f"got {float(got.reshape(-1)[w])!r} ref {float(ref.reshape(-1)[w])!r} err {float(err.reshape(-1)[w]):.3e} "
                             f"bound {float(bound.reshape(-1)[w]):.3e}")
    if ceiling is not None:
        top = float((k * unit / (1.0 + ref.abs())).max())
        print(f"CEIL {family} {top:.3g} {what}")
        assert top <= ceiling, f"{family} {what}: chosen fp32 bound {top:.3e} (1 + |ref|) above {ceiling} (1 + |ref|)"


# ---- geometry of the launch (csrc/groupnorm.hip), restated for the bounds ------------------------------------------------------------
def _geometry(n, hw, c, unsplit=False):
    """-> m (values a thread adds per channel and workgroup), addends per accumulator of the backward sums"""
    rpp = 256 // (c // 8)                            # pixel rows per pass of a workgroup
    rpb = 1024 if hw > 4096 else 64                  # pixels per workgroup
    nb = -(-hw // rpb)
    m = -(-min(rpb, hw) // rpp)
    m_stats = -(-hw // rpp) if unsplit else m
    acc = m + min(rpp, rpb, hw) + nb * n             # registers, live LDS rows, blocks and images
    return m_stats, acc


def _ch(v, c):
    """[N, G] -> [N, 1, C]"""
    return v.repeat_interleave(c // v.shape[1], dim=1)[:, None, :]


def _gmean(t, g):
    """[N, P, C] -> mean per (n, group) as [N, 1, C]"""
    n, p, c = t.shape
    return _ch(t.reshape(n, p, g, c // g).mean(dim=(1, 3)), c)


class Operands:
    """x, dy, addend [N, HW, C] rounded to the tensor type, gamma / beta and accumulator starts in fp32 -- host fp32 tensors"""

    def __init__(self, n, hw, c, g, dtype, seed, musig=1.0 / 3.0, special=False):
        rs = np.random.RandomState(seed)
        sigma = 1.5
        x = sigma * rs.standard_normal((n, hw, c)) + musig * sigma
        if special:                                  # one constant group at a non-dyadic value, one group of zeros
            cpg = c // g
            x[0, :, 5 * cpg:6 * cpg] = 0.1
            x[n - 1, :, 9 * cpg:10 * cpg] = 0.0
        self.x = _rnd(x, dtype)
        del x
        self.dy = _rnd(rs.standard_normal((n, hw, c)), dtype)
        self.add = _rnd(rs.standard_normal((n, hw, c)), dtype)
        self.gamma = torch.from_numpy((1 + 0.2 * rs.standard_normal(c)).astype(np.float32))
        self.beta = torch.from_numpy((0.2 * rs.standard_normal(c)).astype(np.float32))
        self.dg0 = torch.from_numpy(rs.standard_normal(c).astype(np.float32))
        self.db0 = torch.from_numpy(rs.standard_normal(c).astype(np.float32))
        self.n, self.hw, self.c, self.g, self.dtype, self.special = n, hw, c, g, dtype, special


@functools.lru_cache(maxsize=2)
def _operands(n, hw, c, g, dtype, musig=1.0 / 3.0, special=False):
    return Operands(n, hw, c, g, dtype, 7 * n + 3 * hw + c + g + int(1000 * musig), musig, special)


# ---- forms ---------------------------------------------------------------------------------------------------------------------------
def _stat_bounds(op, x, m_stats, eps, given=None):
    """reference statistics and their derived bounds.  given = (mean, var) [N, G]: statistics handed to the kernels (no sums of x)"""
    cnt = float(op.hw * (op.c // op.g))
    if given is None:
        s, q, a = M.group_sums(x, op.g)
        mean, var = M.group_mean_var(x, op.g)
        ds, dq = m_stats * U * a, m_stats * U * q
    else:
        mean, var = given
        s, q = mean * cnt, (var + mean * mean) * cnt
        ds = dq = torch.zeros_like(mean)
    rstd = M.rstd_of(var, eps)
    dmean = ds / cnt + U * mean.abs()
    drel = 0.5 * (dq / cnt + 2 * mean.abs() * ds / cnt) / (var + eps) + U
    # what y and the {scale, shift} table carry: the same two expressions with sqrt(m) in place of m -- the m roundings of a thread's
    # sum add like a random walk; the worst case m would put the fp32 bound of y above what test_groupnorm accepts (mu / sigma = 2 on
    # 1024-pixel blocks), so the forms take the expected growth and the measured constant covers the rest
    w = 1.0 / math.sqrt(max(m_stats, 1))
    mu = (w * ds / cnt) / U + mean.abs()
    rho = (0.5 * w * (dq / cnt + 2 * mean.abs() * ds / cnt) / (var + eps)) / U + 1
    return dict(s=s, q=q, ds=ds, dq=dq, mean=mean, var=var, rstd=rstd, dmean=dmean, drel=drel, mu=mu, rho=rho)


def _forward_forms(op, x, st, gamma, beta, kind):
    """z = xhat gamma + beta is evaluated as x sc + sh, sc = rstd gamma, sh = beta - mean sc, each rounded to fp32:
         sc:  |sc| (rho + 1)                                  rho, mu: drstd / rstd and dmean of _stat_bounds in units of 2^-24,
                                                              with sqrt(m) in place of m
         sh:  |sc| mu + |mean sc| (rho + 2) + |sh|
         z:   |xhat gamma| (rho + 1) + |sc| mu + 2 |mean sc| + |sh| + |z|
         y:   sup|act'| (form of z) + |y| (+ z^2 s (1 - s) for swish: the exponential is relative in its argument)"""
    c = op.c
    rho, mu = _ch(st["rho"], c), _ch(st["mu"], c)
    mean, rstd = _ch(st["mean"], c), _ch(st["rstd"], c)
    sc = rstd * gamma
    sh = beta - mean * sc
    f_sc = sc.abs() * (rho + 1)
    f_sh = sc.abs() * mu + (mean * sc).abs() * (rho + 2) + sh.abs()
    y, z, _, _ = M.gn_forward(x, gamma, beta, op.g, 0.0, kind, mean=st["mean"], rstd=st["rstd"])
    xhg = (z - beta).abs()
    f_z = xhg * (rho + 1) + sc.abs() * mu + 2 * (mean * sc).abs() + sh.abs() + z.abs()
    f_y = ACT_SLOPE[kind] * f_z + y.abs()
    if kind == M.ACT_SWISH:
        s = torch.sigmoid(z)
        f_y = f_y + z * z * s * (1 - s)
    return y, f_y, torch.stack([sc, sh], -1)[:, 0], torch.stack([f_sc, f_sh], -1)[:, 0]


def _backward_forms(op, x, dy, add, gamma, beta, kind, mean, rstd, acc, fixed):
    """mean / rstd: the fp32 statistics the forward kernel saved (the reference takes the same values).  G = sup|act'| |dy gamma|:
         dx:     rstd (3 G + |dy gamma| sup|act''| (|xhat gamma| + |z|) + acc (mean_g G + |xhat| mean_g (G |xhat|))) + |addend| + |dx|
                 (fixed statistics: no group means, acc = 0)
         dgamma: (acc + 4) (sum sup|act'| |dy| |xhat| + |start|),  dbeta: (acc + 4) (sum sup|act'| |dy| + |start|)
       acc = addends per accumulator (registers + LDS rows + blocks x images).  LeakyReLU: an element whose z lies within its own
       rounding of the kink may take either slope -- the 0.8 |dy| jump of those elements is allowed on top (absolute)."""
    g, c = op.g, op.c
    dx, dgam, dbet = M.gn_backward(x, dy, gamma, beta, g, kind, mean, rstd, addend=add, fixed_stats=fixed)
    xh = M.normalized(x, mean, rstd)
    z = xh * gamma + beta
    r = _ch(rstd, c)
    big = ACT_SLOPE[kind] * (dy * gamma).abs()
    f_dx = r * (3 * big + (dy * gamma).abs() * ACT_CURV[kind] * ((xh * gamma).abs() + z.abs()))
    if not fixed:
        f_dx = f_dx + r * acc * (_gmean(big, g) + xh.abs() * _gmean(big * xh.abs(), g))
    f_dx = f_dx + dx.abs() + (0.0 if add is None else add.abs())
    f_dg = (acc + 4) * (ACT_SLOPE[kind] * (dy.abs() * xh.abs()).sum(dim=(0, 1)) + op.dg0.double().to(x.device).abs())
    f_db = (acc + 4) * (ACT_SLOPE[kind] * dy.abs().sum(dim=(0, 1)) + op.db0.double().to(x.device).abs())
    jump = None
    if kind == M.ACT_LRELU:
        near = z.abs() <= 8 * U * ((xh * gamma).abs() + z.abs() + beta.abs())
        if bool(near.any()):
            j = 0.8 * dy.abs() * near
            jg = j * gamma.abs()
            jx = r * jg if fixed else r * (jg + _gmean(jg, g) + xh.abs() * _gmean(jg * xh.abs(), g))
            jump = (jx, (j * xh.abs()).sum(dim=(0, 1)), j.sum(dim=(0, 1)))
    return dx, dgam, dbet, f_dx, f_dg, f_db, jump


# ---- one case through every entry ---------------------------------------------------------------------------------------------------
def _run_case(dev, op, det, acts=ACTS, eps=EPS, ceiling=CEIL_NORM, unsplit=False, given=None, fixed=False, ref_dev="cpu",
              expect_bwd_error=False, addends=(False, True), tag=""):
    """statistics, mean / rstd, the {scale, shift} table, y, dx, dgamma, dbeta of one shape, per element.  given: (mean, var) [N, G]
    handed to the kernels as {sum, sum of squares} instead of dvq_gn_stats' own.  Returns the device outputs of the last activation"""
    from dynamicvectorquantization_amd._lib import DvqError
    n, hw, c, g, dtype = op.n, op.hw, op.c, op.g, op.dtype
    m_stats, acc = _geometry(n, hw, c, unsplit)
    tag = f"{tag}({n}, {hw}, {c}, {g}) {'bf16' if dtype == torch.bfloat16 else 'fp32'} det {int(det)}"
    x, dy, add = (t.to(ref_dev).double() for t in (op.x, op.dy, op.add))
    gamma, beta = op.gamma.to(ref_dev).double(), op.beta.to(ref_dev).double()
    st = _stat_bounds(op, x, m_stats, eps, None if given is None else tuple(t.to(ref_dev).double() for t in given))
    xt, dyt, addt = (t.to(dev).to(dtype) for t in (op.x, op.dy, op.add))
    gt, bt = op.gamma.to(dev), op.beta.to(dev)
    out = {}
    with _mode(det) as K:
        if given is None:
            stats = K.gn_stats(xt, g)
            _pin("stats", stats[..., 0], st["s"], st["ds"] / U, what="sum " + tag)
            _pin("stats", stats[..., 1], st["q"], st["dq"] / U, what="sum of squares " + tag)
        else:
            stats = torch.stack([st["s"], st["q"]], -1).to(dev).contiguous()
        ss, mr2 = K.gn_scale_shift(xt, gt, bt, g, eps, stats=stats)
        for kind in acts:
            atag = f"{ACT_NAME[kind]} {tag}"
            y, mr = K.gn_forward(xt, gt, bt, g, eps, kind, stats=stats)
            assert torch.equal(mr, mr2), f"{atag}: mean_rstd of gn_forward and gn_scale_shift differ on the same statistics"
            y_ref, f_y, ss_ref, f_ss = _forward_forms(op, x, st, gamma, beta, kind)
            if kind == acts[0]:
                _pin("mean", mr[..., 0], st["mean"], st["dmean"] / U, what=tag)
                _pin("rstd", mr[..., 1], st["rstd"], st["rstd"] * st["drel"] / U, what=tag)
                _pin("scale_shift", ss, ss_ref, f_ss, what=tag)
            _pin("y", y, y_ref, f_y, dtype, ceiling=ceiling, what=atag)
            if op.special:
                _check_zero_group(op, y, kind, atag)
            mean_k, rstd_k = mr[..., 0].to(ref_dev).double(), mr[..., 1].to(ref_dev).double()
            dx0 = None
            for with_add in addends:
                dg, db = op.dg0.to(dev).clone(), op.db0.to(dev).clone()
                if expect_bwd_error:
                    with pytest.raises(DvqError):
                        K.gn_backward(xt, dyt, mr, gt, bt, dg, db, g, kind, addend=addt if with_add else None, fixed_stats=fixed)
                    continue
                dx = K.gn_backward(xt, dyt, mr, gt, bt, dg, db, g, kind, addend=addt if with_add else None, fixed_stats=fixed)
                dx_ref, dg_ref, db_ref, f_dx, f_dg, f_db, jump = _backward_forms(op, x, dy, add if with_add else None, gamma, beta, kind,
                                                                                 mean_k, rstd_k, acc, fixed)
                btag = f"{atag} addend {int(with_add)}"
                jx, jg, jb = jump if jump is not None else (None, None, None)
                _pin("dx", dx, dx_ref, f_dx, dtype, extra=jx, ceiling=ceiling, what=btag)
                _pin("dparam", dg, dg_ref + op.dg0.double().to(ref_dev), f_dg, extra=jg, what="dgamma " + btag)
                _pin("dparam", db, db_ref + op.db0.double().to(ref_dev), f_db, extra=jb, what="dbeta " + btag)
                if with_add and dx0 is not None and det:
                    # the addend joins after dx is formed: one rounding of the stored dx0, one of the sum.  Deterministic mode only:
                    # with the mode off two launches differ in the reduced sums behind the group means
                    unit = BF if dtype == torch.bfloat16 else U
                    d0, d1 = dx0.double(), dx.double()
                    assert bool(((d1 - (d0 + addt.double())).abs() <= unit * (d0.abs() + d1.abs()) + TINY).all()), \
                        f"{btag}: dx with the addend is not dx + addend"
                dx0 = dx if not with_add else dx0
                out.update(dx=dx, dg=dg, db=db)
            out.update(stats=stats, ss=ss, mr=mr, y=y)
    torch.cuda.synchronize()
    return out


def _check_zero_group(op, y, kind, tag):
    """a group of zeros: mean 0, rstd 1 / sqrt(eps) = 1000, xhat = 0, y = act(beta) exactly"""
    cpg = op.c // op.g
    ch = slice(9 * cpg, 10 * cpg)
    got = y[op.n - 1, :, ch].float().cpu()
    beta = op.beta[ch]
    assert bool((got == got[:1]).all()), f"{tag}: the zero group's pixels differ"
    if kind != M.ACT_SWISH:           # swish goes through the hardware exponential: held to its bound by the caller, not bit for bit
        want = beta if kind == M.ACT_NONE else torch.where(beta > 0, beta, torch.tensor(0.2, dtype=torch.float32) * beta)
        want = want.to(op.dtype).float()
        assert torch.equal(got[0], want), f"{tag}: the zero group is not act(beta)"


def _repeatable(dev, op, kind=M.ACT_SWISH, eps=EPS):
    """deterministic mode: two launches of the whole chain are bit-identical"""
    xt, dyt, addt = (t.to(dev).to(op.dtype) for t in (op.x, op.dy, op.add))
    gt, bt = op.gamma.to(dev), op.beta.to(dev)
    runs = []
    with _mode(True) as K:
        for _ in range(2):
            stats = K.gn_stats(xt, op.g)
            y, mr = K.gn_forward(xt, gt, bt, op.g, eps, kind, stats=stats)
            dg, db = op.dg0.to(dev).clone(), op.db0.to(dev).clone()
            dx = K.gn_backward(xt, dyt, mr, gt, bt, dg, db, op.g, kind, addend=addt)
            runs.append((stats, y, mr, dx, dg, db))
    torch.cuda.synchronize()
    for a, b in zip(*runs):
        assert torch.equal(a, b), "deterministic mode: identical launches differ"


def _fin_ok(c, g):
    cpg = c // g
    return cpg & (cpg - 1) == 0 and cpg <= 32


# ---- the dispatch edges -----------------------------------------------------------------------------------------------------------------
# (N, HW, C, G); both modes
EDGES_BOTH = [
    (1, 5000, 8, 8), (2, 35, 8, 1),                                        # one column, 64 of 256 threads live; cpg 1; cpg 8 (N 2)
    (3, 64, 64, 32), (3, 64, 128, 32), (2, 100, 256, 32), (1, 64, 512, 32),  # cpg 2 / 4 / 8 / 16; tail only, one 4-row trip, 16 rows per thread
    (2, 70, 1024, 32),                                                     # cpg 32
    (2, 70, 1032, 129), (2, 70, 40, 5),                                    # rows per pass 1 with 127 idle threads; C % 32 != 0 in the finalize
    (1, 70, 2048, 2048),                                                   # every thread one column, cpg 1
    (2, 1, 128, 32), (2, 35, 128, 32), (2, 64, 128, 32), (2, 65, 128, 32),   # one pixel; partial block; seam; second block of one pixel
    (2, 4096, 64, 32), (2, 4097, 64, 32), (2, 9216, 64, 32), (2, 21 * 1024 + 7, 64, 32),   # 64 / 1024 rows; last block one pixel; 16-stride + tail
]
# C / G not a power of two <= 32: the reduce kernel adds with atomics; deterministic mode refuses the backward
EDGES_ATOMICS = [(2, 65, 96, 32), (2, 33 * 31, 96, 8), (1, 70, 2048, 32)]


def _ids(cases):
    return ["x".join(str(v) for v in s) for s in cases]


@MODES
@DTYPES
@pytest.mark.parametrize("shape", EDGES_BOTH, ids=_ids(EDGES_BOTH))
def test_edges(dev, shape, dtype, det):
    """every activation, addend absent and present, accumulators from non-zero starts"""
    op = _operands(*shape, dtype)
    _run_case(dev, op, det)
    if det:
        _repeatable(dev, op)


@MODES
@DTYPES
@pytest.mark.parametrize("shape", EDGES_ATOMICS, ids=_ids(EDGES_ATOMICS))
def test_edges_atomics_fallback(dev, shape, dtype, det):
    """cpg 3 (a thread's 8 channels in 3 - 4 groups, 252 live threads, 21 rows per pass), 12 and 64: no finalize kernel.  With the mode
    on the statistics and the forward still pass and the backward raises"""
    assert not _fin_ok(shape[2], shape[3])
    op = _operands(*shape, dtype)
    _run_case(dev, op, det, expect_bwd_error=det)


@DTYPES
@pytest.mark.parametrize("shape", [(1, 5000, 16, 16)], ids=_ids([(1, 5000, 16, 16)]))
def test_fixed_statistics(dev, shape, dtype):
    """ActNorm's form: caller-made statistics mean = -loc, var = 1 - eps (rstd = 1), gamma = scale, beta = 0, LeakyReLU;
    the backward drops the statistic terms: dx = rstd gamma dz"""
    n, hw, c, g = shape
    op = Operands(n, hw, c, g, dtype, seed=hw + c)
    op.beta.zero_()
    eps = float(np.float32(1e-5))
    loc = torch.from_numpy(np.random.RandomState(3).standard_normal(c).astype(np.float32))
    given = (-loc.double()[None], torch.full((1, c), 1.0 - eps, dtype=torch.float64))
    for det in (False, True):
        _run_case(dev, op, det, acts=(M.ACT_LRELU, M.ACT_NONE), eps=eps, given=given, fixed=True, tag="fixed ")


@DTYPES
def test_external_statistics(dev, dtype):
    """eval BatchNorm's form: running mean / variance scaled by the count and handed in as {sum, sum of squares}"""
    n, hw, c = 1, 700, 24
    op = _operands(n, hw, c, c, dtype)
    rs = np.random.RandomState(11)
    rm = torch.from_numpy((0.5 + 0.2 * rs.standard_normal(c)).astype(np.float32)).double()          # near the batch's own: x = 1.5 N(0, 1) + 0.5
    rv = torch.from_numpy((2.25 * (0.8 + 0.4 * rs.rand(c))).astype(np.float32)).double()
    eps = float(np.float32(1e-5))
    _run_case(dev, op, False, eps=eps, given=(rm[None], rv[None]), addends=(False,), acts=(M.ACT_LRELU, M.ACT_NONE), tag="external ")
    y_ref = M.bn_eval(op.x, rm, rv, op.gamma, op.beta, eps, M.ACT_LRELU)
    y2, _, _, _ = M.gn_forward(op.x, op.gamma, op.beta, c, eps, M.ACT_LRELU, mean=rm[None], rstd=M.rstd_of(rv, eps)[None])
    assert float((y2 - y_ref).abs().max()) <= 1e-12 * float(y_ref.abs().max())


@DTYPES
@pytest.mark.parametrize("shape", [(3, 4097, 64, 32), (1, 9216, 128, 32)], ids=_ids([(3, 4097, 64, 32), (1, 9216, 128, 32)]))
@pytest.mark.parametrize("workspace", [True, False], ids=["workspace", "no-workspace"])
def test_deterministic_folds(dev, shape, dtype, workspace, monkeypatch):
    """with a registered workspace: per-block partials, per-image terms and ordered folds; with none: the statistics as one workgroup
    per image over every pixel (rpb = HW), the finalize kernel walking the images serially.  Values and bit-repeatability"""
    K = _k()
    op = _operands(*shape, dtype)
    if workspace:
        K.ensure_workspace(dev)
    else:
        _no_workspace(monkeypatch)
    c0 = K.unordered_launches()
    _run_case(dev, op, True, unsplit=not workspace, ceiling=CEIL_NORM if workspace else None, tag="folds ")
    _repeatable(dev, op)
    assert K.unordered_launches() == c0, "deterministic mode took an unordered path"


COND = [(0, False), (2, False), (8, False), (32, False), (0, True)]


@MODES
@DTYPES
@pytest.mark.parametrize("musig,special", COND, ids=["mu0sigma", "mu2sigma", "mu8sigma", "mu32sigma", "constant-and-zero-groups"])
def test_conditioning(dev, musig, special, dtype, det):
    """(2, 9216, 128, 32) at mu / sigma = 0, 2, 8, 32: same forms and constants, the ceiling only up to 2.  One group constant at 0.1
    (variance 0: rstd rests on eps alone), one group of zeros (rstd = 1000, y = act(beta) exactly)"""
    op = _operands(2, 9216, 128, 32, dtype, float(musig), special)
    regular = musig <= 2 and not special
    out = _run_case(dev, op, det, ceiling=CEIL_NORM if regular else None, addends=(False,), tag=f"mu/sigma {musig} ")
    if special:
        mr = out["mr"].cpu()
        assert float(mr[1, 9, 0]) == 0.0 and float(mr[1, 9, 1]) == 1000.0


# operand bytes above 192 MiB: the nontemporal instantiations, which the product's 256 x 256 maps run
NT_CASES = [("fp32-nontemporal", torch.float32, 640 * 615, 128), ("bf16-nontemporal", torch.bfloat16, 640 * 615, 256),
            ("fp32-below-switch", torch.float32, 393000, 128)]


@pytest.mark.parametrize("name,dtype,hw,c", NT_CASES, ids=[t[0] for t in NT_CASES])
def test_nontemporal(dev, name, dtype, hw, c):
    """201 523 200 bytes (> 192 x 2^20) in fp32 at C 128 and in bf16 at C 256; 201 216 000 stays below.  Swish, forward and backward
    with the addend; the fp64 reference runs on the device for these three"""
    nbytes = hw * c * (4 if dtype == torch.float32 else 2)
    assert (nbytes > 192 * 2 ** 20) == ("nontemporal" in name)
    op = Operands(1, hw, c, 32, dtype, seed=hw + c)
    _run_case(dev, op, False, acts=(M.ACT_SWISH,), addends=(True,), ref_dev=dev, tag=name + " ")


# ---- rejections ahead of any launch ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,c,g", [(1, 12, 4), (1, 2056, 8), (1, 96, 5), (65536, 8, 8)], ids=["C12", "C2056", "C96-G5", "N65536"])
def test_rejections(dev, n, c, g):
    """C % 8 != 0; C / 8 > 256; C % G != 0; N > 65535 (the grid's y limit): DvqError from every entry, nothing launched"""
    K = _k()
    from dynamicvectorquantization_amd._lib import DvqError
    x = torch.zeros(n, 1, c, device=dev)
    gamma, beta = torch.ones(c, device=dev), torch.zeros(c, device=dev)
    gg = g if c % g == 0 else 1
    stats = torch.zeros(n, gg, 2, dtype=torch.float64, device=dev)
    mr = torch.zeros(n, gg, 2, device=dev)
    dg, db = torch.zeros(c, device=dev), torch.zeros(c, device=dev)
    for det in (False, True):
        with _mode(det):
            with pytest.raises(DvqError):
                K.gn_stats(x, g)
            with pytest.raises(DvqError):
                K.gn_forward(x, gamma, beta, g, EPS, 1, stats=stats)
            with pytest.raises(DvqError):
                K.gn_scale_shift(x, gamma, beta, g, EPS, stats=stats)
            with pytest.raises(DvqError):
                K.gn_backward(x, x, mr, gamma, beta, dg, db, g, 1)
    torch.cuda.synchronize()
    assert float(dg.abs().sum()) == 0.0 and float(db.abs().sum()) == 0.0


# ---- the layers -----------------------------------------------------------------------------------------------------------------------
def _layer_inputs(c, dtype, seed):
    rs = np.random.RandomState(seed)
    x = _rnd(1.5 * rs.standard_normal((2, 9, 7, c)) + 0.5, dtype)
    dy = _rnd(rs.standard_normal((2, 9, 7, c)), dtype)
    add = _rnd(rs.standard_normal((2, 9, 7, c)), dtype)
    gamma = torch.from_numpy((1 + 0.2 * rs.standard_normal(c)).astype(np.float32))
    beta = torch.from_numpy((0.2 * rs.standard_normal(c)).astype(np.float32))
    return x, dy, add, gamma, beta


def _layer_op(x, dy, add, gamma, beta, n, hw, c, g, dtype, dg0, db0):
    op = Operands.__new__(Operands)
    op.x, op.dy, op.add = x.reshape(n, hw, c), dy.reshape(n, hw, c), add.reshape(n, hw, c)
    op.gamma, op.beta, op.dg0, op.db0 = gamma, beta, dg0, db0
    op.n, op.hw, op.c, op.g, op.dtype, op.special = n, hw, c, g, dtype, False
    return op


@DTYPES
def test_layer_normalize(dev, dtype):
    """Normalize.fwd / prep / bwd(addend) at (2, 9, 7, 64), G 32, swish fused; the parameter gradients add into non-zero .grad"""
    from dynamicvectorquantization_amd.layers import Normalize, Tape
    c, g = 64, 32
    x, dy, add, gamma, beta = _layer_inputs(c, dtype, 41)
    rs = np.random.RandomState(42)
    dg0, db0 = (torch.from_numpy(rs.standard_normal(c).astype(np.float32)) for _ in range(2))
    op = _layer_op(x, dy, add, gamma, beta, 2, 63, c, g, dtype, dg0, db0)
    mod = Normalize(c).to(dev)
    with torch.no_grad():
        mod.weight.copy_(gamma.to(dev))
        mod.bias.copy_(beta.to(dev))
    mod.weight.grad, mod.bias.grad = dg0.to(dev), db0.to(dev)
    xt, dyt, addt = (t.to(dev).to(dtype) for t in (x, dy, add))
    tape, tape2 = Tape(), Tape()
    y = mod.fwd(xt, tape, silu=True)
    ss = mod.prep(xt, tape2)
    dx = mod.bwd(dyt, tape, addend=addt)
    m_stats, acc = _geometry(2, 63, c)
    x64, dy64, add64 = op.x.double(), op.dy.double(), op.add.double()
    st = _stat_bounds(op, x64, m_stats, EPS)
    y_ref, f_y, ss_ref, f_ss = _forward_forms(op, x64, st, gamma.double(), beta.double(), M.ACT_SWISH)
    _pin("y", y.reshape(2, 63, c), y_ref, f_y, dtype, ceiling=CEIL_NORM, what="Normalize.fwd")
    _pin("scale_shift", ss, ss_ref, f_ss, what="Normalize.prep")
    for t in (tape, tape2):
        _pin("mean", t.s["mr"][..., 0], st["mean"], st["dmean"] / U, what="Normalize")
        _pin("rstd", t.s["mr"][..., 1], st["rstd"], st["rstd"] * st["drel"] / U, what="Normalize")
    mr = tape.s["mr"].cpu().double()
    dx_ref, dg_ref, db_ref, f_dx, f_dg, f_db, _ = _backward_forms(op, x64, dy64, add64, gamma.double(), beta.double(), M.ACT_SWISH,
                                                                  mr[..., 0], mr[..., 1], acc, False)
    _pin("dx", dx.reshape(2, 63, c), dx_ref, f_dx, dtype, ceiling=CEIL_NORM, what="Normalize.bwd")
    _pin("dparam", mod.weight.grad, dg_ref + dg0.double(), f_dg, what="Normalize dgamma")
    _pin("dparam", mod.bias.grad, db_ref + db0.double(), f_db, what="Normalize dbeta")


@DTYPES
def test_layer_batchnorm(dev, dtype):
    """BatchNorm2d at (2, 9, 7, 16) with LeakyReLU fused: training forward and backward, the running statistics and
    num_batches_tracked, then eval mode on the updated buffers"""
    from dynamicvectorquantization_amd import kernels as K
    from dynamicvectorquantization_amd.layers import BatchNorm2d, Tape
    c = 16
    x, dy, add, gamma, beta = _layer_inputs(c, dtype, 43)
    rs = np.random.RandomState(44)
    dg0, db0 = (torch.from_numpy(rs.standard_normal(c).astype(np.float32)) for _ in range(2))
    rm0 = torch.from_numpy(rs.standard_normal(c).astype(np.float32))
    rv0 = torch.from_numpy((0.5 + rs.rand(c)).astype(np.float32))
    op = _layer_op(x, dy, add, gamma, beta, 1, 126, c, c, dtype, dg0, db0)
    mod = BatchNorm2d(c).to(dev)
    mod.act = K.ACT_LRELU
    with torch.no_grad():
        mod.weight.copy_(gamma.to(dev))
        mod.bias.copy_(beta.to(dev))
        mod.running_mean.copy_(rm0.to(dev))
        mod.running_var.copy_(rv0.to(dev))
    mod.weight.grad, mod.bias.grad = dg0.to(dev), db0.to(dev)
    xt, dyt = x.to(dev).to(dtype), dy.to(dev).to(dtype)
    eps = float(np.float32(mod.eps))
    mod.train()
    tape = Tape()
    y = mod.fwd(xt, tape)
    dx = mod.bwd(dyt, tape)
    m_stats, acc = _geometry(1, 126, c)
    x64, dy64 = op.x.double(), op.dy.double()
    st = _stat_bounds(op, x64, m_stats, eps)
    y_ref, f_y, _, _ = _forward_forms(op, x64, st, gamma.double(), beta.double(), M.ACT_LRELU)
    assert float((y_ref.reshape(x.shape) - M.bn_train(x, gamma, beta, eps, M.ACT_LRELU)).abs().max()) <= 1e-12 * float(y_ref.abs().max())
    _pin("y", y.reshape(1, 126, c), y_ref, f_y, dtype, ceiling=CEIL_NORM, what="BatchNorm2d train")
    mr = tape.s["mr"].cpu().double()
    dx_ref, dg_ref, db_ref, f_dx, f_dg, f_db, jump = _backward_forms(op, x64, dy64, None, gamma.double(), beta.double(), M.ACT_LRELU,
                                                                     mr[..., 0], mr[..., 1], acc, False)
    jx, jg, jb = jump if jump is not None else (None, None, None)
    _pin("dx", dx.reshape(1, 126, c), dx_ref, f_dx, dtype, extra=jx, ceiling=CEIL_NORM, what="BatchNorm2d bwd")
    _pin("dparam", mod.weight.grad, dg_ref + dg0.double(), f_dg, extra=jg, what="BatchNorm2d dgamma")
    _pin("dparam", mod.bias.grad, db_ref + db0.double(), f_db, extra=jb, what="BatchNorm2d dbeta")
    # running statistics: fp64 on the device from the kernel's sums, rounded once and blended in fp32
    rm_ref, rv_ref = M.bn_running_update(x, rm0, rv0, mod.momentum)
    cnt = 126.0
    d_mean = st["dmean"][0]
    d_var = (st["dq"][0] / cnt + 2 * st["mean"][0].abs() * st["ds"][0] / cnt) * (cnt / (cnt - 1)) + U * st["var"][0]
    _pin("mean", mod.running_mean, rm_ref, (mod.momentum * d_mean + 2 * U * (rm_ref.abs() + rm0.double().abs())) / U, what="running_mean")
    _pin("mean", mod.running_var, rv_ref, (mod.momentum * d_var + 2 * U * (rv_ref.abs() + rv0.double().abs())) / U, what="running_var")
    assert int(mod.num_batches_tracked) == 1
    # eval mode: a per-channel affine map of the (updated) buffers
    mod.eval()
    rm1, rv1 = mod.running_mean.cpu().double(), mod.running_var.cpu().double()
    ye = mod.fwd(xt, None)
    assert int(mod.num_batches_tracked) == 1 and torch.equal(mod.running_mean.cpu().double(), rm1)
    ste = _stat_bounds(op, x64, 0, eps, given=(rm1[None], rv1[None]))
    ye_ref, f_ye, _, _ = _forward_forms(op, x64, ste, gamma.double(), beta.double(), M.ACT_LRELU)
    assert float((ye_ref.reshape(x.shape) - M.bn_eval(x, rm1, rv1, gamma, beta, eps, M.ACT_LRELU)).abs().max()) <= 1e-12 * float(ye_ref.abs().max())
    _pin("y", ye.reshape(1, 126, c), ye_ref, f_ye, dtype, ceiling=CEIL_NORM, what="BatchNorm2d eval")


@DTYPES
def test_layer_actnorm(dev, dtype):
    """ActNorm at (2, 9, 7, 16) after a loaded state (no data-dependent initialisation): h = LeakyReLU(scale (x + loc)),
    d scale = sum dz (x + loc), d loc = scale sum dz, dx = scale dz"""
    from dynamicvectorquantization_amd import kernels as K
    from dynamicvectorquantization_amd.layers import ActNorm, Tape
    c = 16
    x, dy, add, scale, loc = _layer_inputs(c, dtype, 45)
    zero = torch.zeros(c)
    op = _layer_op(x, dy, add, scale, zero, 1, 126, c, c, dtype, zero, zero)
    src = ActNorm(c)
    with torch.no_grad():
        src.loc.copy_(loc.view(1, c, 1, 1))
        src.scale.copy_(scale.view(1, c, 1, 1))
        src.initialized.fill_(1)
    mod = ActNorm(c)
    mod.load_state_dict(src.state_dict())
    mod = mod.to(dev)
    mod.act = K.ACT_LRELU
    mod.train()
    xt, dyt = x.to(dev).to(dtype), dy.to(dev).to(dtype)
    tape = Tape()
    y = mod.fwd(xt, tape)
    assert torch.equal(mod.loc.detach().cpu().view(c), loc) and torch.equal(mod.scale.detach().cpu().view(c), scale), "re-initialised"
    dx = mod.bwd(dyt, tape)
    eps = float(np.float32(mod.EPS))
    x64, dy64 = op.x.double(), op.dy.double()
    st = _stat_bounds(op, x64, 0, eps, given=(-loc.double()[None], torch.full((1, c), 1.0 - eps, dtype=torch.float64)))
    y_ref, f_y, _, _ = _forward_forms(op, x64, st, scale.double(), zero.double(), M.ACT_LRELU)
    want = M.actnorm_forward(x, loc, scale, M.ACT_LRELU)
    assert float((y_ref.reshape(x.shape) - want).abs().max()) <= 1e-9 * float(want.abs().max())       # rstd = 1 to 1e-11 only
    _pin("y", y.reshape(1, 126, c), want.reshape(1, 126, c), f_y, dtype, ceiling=CEIL_NORM, what="ActNorm fwd")
    mr = tape.s["mr"].cpu().double()
    dx_ref, dsc_ref, dsum_ref, f_dx, f_dg, f_db, jump = _backward_forms(op, x64, dy64, None, scale.double(), zero.double(), M.ACT_LRELU,
                                                                        mr[..., 0], mr[..., 1], _geometry(1, 126, c)[1], True)
    jx, jg, jb = jump if jump is not None else (None, None, None)
    _pin("dx", dx.reshape(1, 126, c), dx_ref, f_dx, dtype, extra=jx, ceiling=CEIL_NORM, what="ActNorm bwd")
    _pin("dparam", mod.scale.grad.view(c), dsc_ref, f_dg, extra=jg, what="ActNorm dscale")
    _pin("dparam", mod.loc.grad.view(c), dsum_ref * scale.double(), f_db * scale.double().abs() + (dsum_ref * scale.double()).abs(),
         extra=None if jb is None else jb * scale.double().abs(), what="ActNorm dloc")
