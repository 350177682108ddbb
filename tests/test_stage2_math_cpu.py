"""tests/stage2_math.py against torch in fp64 (no GPU): the references the device tests of test_gpu_stage2_kernels.py compare with are
themselves checked against F.layer_norm, F.gelu, torch.softmax, F.cross_entropy, F.embedding and autograd.

Agreement: 1e-12 relative, |a - ref| <= 1e-12 (|ref| + mean|ref|) per element -- the second term because both sides are fp64 sums whose
cancelling elements carry the rounding of the tensor's typical magnitude, not of their own.  The dropout hash has no independent CPU
source: only its kept fraction and its dependence on the seed are checked here, the device comparison is its real check."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import stage2_math as M

RTOL = 1e-12


def _close(a, ref):
    a, ref = np.asarray(a, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert a.shape == ref.shape
    bound = RTOL * (np.abs(ref) + np.abs(ref).mean())
    bad = np.abs(a - ref) > bound
    assert not bad.any(), f"{int(bad.sum())} elements differ, worst {np.abs(a - ref).max():.3e}"


def _t(a, grad=False):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).requires_grad_(grad)


@pytest.mark.parametrize("rows,c", [(1, 8), (7, 72), (3, 1032)])
@pytest.mark.parametrize("with_res", [False, True])
def test_layernorm(rows, c, with_res):
    rs = np.random.RandomState(rows + c)
    x = rs.standard_normal((rows, c)) * 1.5 + 2.0
    gamma, beta = 1 + 0.2 * rs.standard_normal(c), 0.2 * rs.standard_normal(c)
    dy, dres = rs.standard_normal((rows, c)), rs.standard_normal((rows, c))
    y, mean, rstd = M.layernorm_fwd(x, gamma, beta, 1e-5)
    xt, gt, bt = _t(x, True), _t(gamma, True), _t(beta, True)
    yt = F.layer_norm(xt, (c,), gt, bt, 1e-5)
    _close(y, yt.detach().numpy())
    _close(mean, x.mean(1))
    _close(rstd, 1.0 / np.sqrt(x.var(1) + 1e-5))
    loss = (yt * _t(dy)).sum()
    if with_res:
        loss = loss + (xt * _t(dres)).sum()          # the residual stream: its gradient reaches x unchanged
    loss.backward()
    dx, dg, db = M.layernorm_bwd(x, dy, gamma, 1e-5, dres=dres if with_res else None)
    _close(dx, xt.grad.numpy())
    _close(dg, gt.grad.numpy())
    _close(db, bt.grad.numpy())
    dx2, dg2, _ = M.layernorm_bwd(x, dy, gamma, 1e-5, dres=dres if with_res else None, mean=mean, rstd=rstd)
    assert np.array_equal(dx, dx2) and np.array_equal(dg, dg2)


def test_gelu():
    """x in [-3, 8] per element (torch forms 1 + erf, which loses relative precision further left); the left tail against the
    magnitude of the whole tensor"""
    rs = np.random.RandomState(3)
    for lo, hi in ((-3.0, 8.0), (-9.0, 9.0)):
        x = np.concatenate([rs.uniform(lo, hi, 4096), [0.0, 1e-30, -1e-30, 1e-4, -1e-4]])
        xt = _t(x, True)
        yt = F.gelu(xt)
        yt.sum().backward()
        _close(M.gelu(x), yt.detach().numpy())
        _close(M.gelu_grad(x), xt.grad.numpy())


@pytest.mark.parametrize("rows,length", [(1, 1), (7, 65), (3, 200)])
@pytest.mark.parametrize("scale", [0.125, -1 / 0.37])
def test_softmax_rows(rows, length, scale):
    rs = np.random.RandomState(rows * length)
    s, dp = rs.standard_normal((rows, length)) * 3, rs.standard_normal((rows, length))
    s[0, :] = np.sign(rs.standard_normal(length)) * 80.0 / abs(scale)
    st = _t(s, True)
    pt = torch.softmax(st * scale, dim=1)
    p = M.softmax_rows(s, scale)
    _close(p, pt.detach().numpy())
    (pt * _t(dp)).sum().backward()
    _close(M.softmax_rows_bwd(p, dp, scale), st.grad.numpy())


@pytest.mark.parametrize("rows,length,tq,offset", [(2, 1, 1, 0), (260, 65, 65, 0), (12, 70, 3, 67), (4, 10, 4, 9)])
def test_softmax_causal(rows, length, tq, offset):
    rs = np.random.RandomState(rows + length)
    s = rs.standard_normal((rows, length)) * 3
    r, c = np.arange(rows)[:, None], np.arange(length)[None, :]
    masked = c > (r % tq) + offset
    ref = torch.softmax(_t(s * 0.3).masked_fill(torch.from_numpy(masked), float("-inf")), dim=1).numpy()
    got = M.softmax_causal(s, tq, offset, 0.3)
    _close(got, ref)
    assert (got[masked] == 0.0).all()
    assert np.array_equal(M.causal_valid(rows, length, tq, offset), (~masked).sum(1))


@pytest.mark.parametrize("v,ldl", [(5, 5), (67, 72), (1027, 1032)])
def test_cross_entropy(v, ldl):
    rs = np.random.RandomState(v)
    rows = 7
    logits = np.full((rows, ldl), 30.0)
    logits[:, :v] = rs.standard_normal((rows, v)) * 3
    logits[3, :v] = -60.0
    logits[3, 1] = 60.0
    target = rs.randint(0, v, rows)
    target[0], target[1] = v - 1, 0
    target[2::3] = -100
    lt = _t(logits[:, :v].copy(), True)
    ref = F.cross_entropy(lt, torch.from_numpy(target), reduction="sum", ignore_index=-100)
    (ref * 0.37).backward()
    loss, count, d = M.cross_entropy(logits, v, target, -100, 0.37)
    _close(np.array([loss]), np.array([float(ref.detach())]))
    assert count == int((target != -100).sum())
    _close(d[:, :v], lt.grad.numpy())
    assert (d[:, v:] == 0.0).all() and (d[target == -100] == 0.0).all()
    loss0, count0, d0 = M.cross_entropy(logits, v, np.full(rows, -100), -100, 0.37)
    assert loss0 == 0.0 and count0 == 0 and not d0.any()


@pytest.mark.parametrize("shared", [False, True])
@pytest.mark.parametrize("t0", [0, 4])
def test_embedding(shared, t0):
    rs = np.random.RandomState(9 + t0)
    b, ln, ttot, c, v, pad = 3, 5, 9, 8, 11, 2
    idx = rs.randint(0, v, (ln,) if shared else (b, ln))
    idx.reshape(-1)[0] = pad
    table, out0 = rs.standard_normal((v, c)), rs.standard_normal((b, ttot, c))
    idx2 = torch.from_numpy(np.broadcast_to(idx, (b, ln)).copy())
    tt = _t(table, True)
    e = F.embedding(idx2, tt, padding_idx=pad)
    for acc in (False, True):
        ref = out0.copy()
        ref[:, t0:t0 + ln] = ref[:, t0:t0 + ln] * (1.0 if acc else 0.0) + e.detach().numpy()
        _close(M.embed_gather(idx, table, out0, t0, acc), ref)
    dout = rs.standard_normal((b, ttot, c))
    (e * _t(dout[:, t0:t0 + ln])).sum().backward()
    start = rs.standard_normal((v, c))
    got = M.embed_scatter_add(idx, dout, start, t0, padding_idx=pad)
    _close(got - start, tt.grad.numpy())
    assert np.array_equal(got[pad], start[pad])
    hits = M.embed_hits(idx, b, v, pad)
    assert hits[pad] == 0 and hits.sum() == int((idx2.numpy() != pad).sum())


def test_bf16_round():
    rs = np.random.RandomState(1)
    x = np.concatenate([rs.standard_normal(4096) * 10.0 ** rs.randint(-20, 20, 4096), [0.0, 1.00390625, 1.01171875, -3.0]]).astype(np.float32)
    assert np.array_equal(M.bf16_round(x), torch.from_numpy(x).to(torch.bfloat16).float().numpy())


def test_dropout_mask_statistics():
    n = 1 << 20
    masks = []
    for p in (0.1, 0.5):
        for seed in (17, (1 << 33) + 5):
            keep = M.dropout_keep(n, p, seed)
            kept, sigma = int(keep.sum()), np.sqrt(n * p * (1 - p))
            assert abs(kept - n * (1 - p)) <= 5 * sigma, (p, seed, kept)
            masks.append(keep)
    assert (masks[0] != masks[1]).any() and (masks[2] != masks[3]).any()
    assert M.dropout_keep(64, 0.0, 17).all()
    # the element index enters through both of its words, and a range that starts later is the same mask shifted
    assert np.array_equal(M.dropout_keep(64, 0.5, 17, start=8), M.dropout_keep(72, 0.5, 17)[8:])
    assert (M.dropout_keep(4096, 0.5, 17, start=1 << 32) != M.dropout_keep(4096, 0.5, 17)).any()
    assert M.dropout_seed(17) != M.dropout_seed(17 + (1 << 32)) and M.dropout_seed(17)[0] % 2 == 1
