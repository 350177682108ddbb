"""GPU tests of the sample-set metrics (docs/design/32-sample-set-metrics.md): dvq_pair_scan and dvq_feat_moments against the fp64
restatements of tests/sampleset_math.py, their edges and reproducibility, evaluate.sample_set_metrics end to end and the model path
(DualGrainVQModel.pooled_features, evaluate.evaluate_samples).

Accuracy: every distance is held to sampleset_math.GRANTED (4 x the CPU-measured deviation of the numpy float32 restatement of the
kernel's staging from fp64) in units of |a|^2 + |b|^2; decisions (counts, radius tests, indices) are held exactly outside a band of
sampleset_math.BAND = 1e-5 of the same unit, and a case in which more than 2 % of the rows have an in-band pair fails as vacuous."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import sampleset_math as SM

pytestmark = pytest.mark.gpu


def _dev(x, dev):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev)


@functools.lru_cache(maxsize=None)
def scan_case(na, nb, d, k):
    """a = the centred fake set [na, d], b = the centred real set [nb, d], the reals' k-th-neighbour radii (fp32, exact inputs of the
    scan) and the fp64 reference of the F|R scan with one more neighbour than asked (the gap behind the last one)"""
    real, fake = SM.make_sets(nb, na, d, seed=SM.case_seed(na, nb, d))
    xr, xf = SM.centre(real, fake)
    kr = min(k, nb - 1)
    rad = SM.pair_scan_ref(xr, xr, kr, exclude_diag=True)[0][:, kr - 1].astype(np.float32)
    d2 = SM.d2_fp64(xf, xr)
    kth2, idx, count = SM.pair_scan_ref(xf, xr, min(k + 1, nb), rad2_b=rad, d2=d2)
    return dict(real=real, fake=fake, a=xf, b=xr, rad=rad, d2=d2, scale=SM.norm_scale(xf, xr), kth2=kth2, idx=idx, count=count)


def check_scan(c, k, kth2, idx, count, exclude_diag=False, label=""):
    """kth2 / idx / count of a scan of c's pair against its fp64 reference (see the module docstring)"""
    d2, scale = c["d2"], c["scale"]
    na, nb = d2.shape
    ref_k, ref_i, ref_c = SM.pair_scan_ref(c["a"], c["b"], min(k + 1, nb), rad2_b=c["rad"], exclude_diag=exclude_diag, d2=d2)
    kth2, idx = kth2.cpu().numpy().astype(np.float64), idx.cpu().numpy()
    assert kth2.shape == (na, k) and idx.shape == (na, k) and idx.dtype == np.int64
    nvalid = min(k, nb - int(exclude_diag))
    assert np.isinf(kth2[:, nvalid:]).all() and (idx[:, nvalid:] == -1).all()
    assert ((idx[:, :nvalid] >= 0) & (idx[:, :nvalid] < nb)).all()
    assert (np.diff(kth2[:, :nvalid], axis=1) >= 0).all()
    # an order statistic of perturbed values moves by at most the largest perturbation among the values that can reach it: the pairs
    # of the row within the band of its k-th distance
    last = ref_k[:, nvalid - 1]
    reach = d2 <= last[:, None] + SM.BAND * scale
    unit = np.where(reach, scale, 0.0).max(axis=1)
    err = np.abs(kth2[:, :nvalid] - ref_k[:, :nvalid]) / unit[:, None]
    print(f"{label} kth2: worst deviation {err.max():.3e} of (|a|^2 + |b|^2), granted {SM.GRANTED:.3e}")
    assert err.max() <= SM.GRANTED
    # the computed distance of the pair a row reports is that pair's distance
    rows = np.arange(na)[:, None]
    own = np.abs(kth2[:, :nvalid] - d2[rows, idx[:, :nvalid]]) / scale[rows, idx[:, :nvalid]]
    assert own.max() <= SM.GRANTED
    # indices: exact wherever both gaps around the rank exceed the band; exact ties (gap 0) follow the lower index, which the reference
    # (a stable sort) already encodes -- those are compared too
    padded = np.concatenate([np.full((na, 1), -np.inf), ref_k], axis=1)              # ranks -1 .. nvalid (or beyond)
    if padded.shape[1] < nvalid + 2:
        padded = np.concatenate([padded, np.full((na, nvalid + 2 - padded.shape[1]), np.inf)], axis=1)
    gap_lo = padded[:, 1:nvalid + 1] - padded[:, 0:nvalid]
    gap_hi = padded[:, 2:nvalid + 2] - padded[:, 1:nvalid + 1]
    tie_lo, tie_hi = gap_lo == 0.0, gap_hi == 0.0
    clear = ((gap_lo > SM.BAND * unit[:, None]) | tie_lo) & ((gap_hi > SM.BAND * unit[:, None]) | tie_hi)
    if not exclude_diag and not (tie_lo | tie_hi).any():
        assert clear.mean() > 0.9, "too few ranks are clear of the band for the index check to mean anything"
    assert (idx[:, :nvalid][clear] == ref_i[:, :nvalid][clear]).all()
    if count is not None:
        count = count.cpu().numpy()
        band = SM.in_band(d2, c["rad"], scale, exclude_diag=exclude_diag)
        rows_in = band.any(axis=1)
        print(f"{label} count: {int(rows_in.sum())} of {na} rows have an in-band pair; largest |count - ref| {np.abs(count - ref_c).max()}")
        assert rows_in.mean() <= 0.02, "vacuous: too many rows are excused by the band"
        assert (np.abs(count - ref_c) <= band.sum(axis=1)).all()


@pytest.mark.parametrize("na,nb,d,k", SM.PAIR_CASES + SM.PAIR_EDGE_CASES, ids=lambda v: str(v))
def test_pair_scan_matches_fp64(dev, na, nb, d, k):
    """the issue's six shapes, then the kernel's own edges (sampleset_math.PAIR_EDGE_CASES says why each): one exact tile / chunk and one
    past it, b split in two and in nine, D % 4 != 0 (scalar loads) and D % 4 == 0 (16-byte loads)"""
    from dynamicvectorquantization_amd import kernels as K
    c = scan_case(na, nb, d, k)
    kth2, idx, count = K.pair_scan(_dev(c["a"], dev), _dev(c["b"], dev), k, rad2_b=_dev(c["rad"], dev))
    check_scan(c, k, kth2, idx, count, label=f"{(na, nb, d, k)}")


def test_pair_scan_exclude_diag_on_and_off(dev):
    """a set against itself: with the diagonal every row's nearest is itself at distance 0 (clamped: the GEMM form may come out
    negative, and may come out a rounding above 0); without it the reference's neighbours.  130 rows: the diagonal crosses into the second tile and the second split"""
    from dynamicvectorquantization_amd import kernels as K
    c0 = scan_case(33, 130, 256, 5)
    d2 = SM.d2_fp64(c0["b"], c0["b"])
    # radii off the set's own k-th distances (x 1.37): with the exact ones every row IS some pair's threshold, in band by construction
    c = dict(a=c0["b"], b=c0["b"], rad=(c0["rad"] * np.float32(1.37)).astype(np.float32), d2=d2, scale=SM.norm_scale(c0["b"], c0["b"]))
    x, rad = _dev(c["b"], dev), _dev(c["rad"], dev)
    kth2, idx, count = K.pair_scan(x, x, 5, rad2_b=rad, exclude_diag=False)
    self_scale = np.diag(c["scale"])                     # a row against itself: 0 up to the GEMM form's error, never negative
    assert (idx[:, 0].cpu().numpy() == np.arange(130)).all() and (kth2 >= 0).all()
    assert (kth2[:, 0].cpu().numpy() <= SM.GRANTED * self_scale).all()
    check_scan(c, 5, kth2, idx, count, exclude_diag=False, label="self, diagonal kept")
    kth2x, idxx, countx = K.pair_scan(x, x, 5, rad2_b=rad, exclude_diag=True)
    assert (idxx.cpu().numpy() != np.arange(130)[:, None]).all()
    check_scan(c, 5, kth2x, idxx, countx, exclude_diag=True, label="self, diagonal skipped")
    # the same computed distances either way: dropping the diagonal shifts the list by one and lowers every count by one (d2 = 0 <= radius)
    assert torch.equal(kth2[:, 1:], kth2x[:, :4]) and torch.equal(idx[:, 1:], idxx[:, :4]) and torch.equal(count - 1, countx)


def test_pair_scan_fewer_candidates_than_k(dev):
    from dynamicvectorquantization_amd import kernels as K
    rng = np.random.default_rng(5)
    a, b = rng.normal(size=(6, 9)).astype(np.float32), rng.normal(size=(3, 9)).astype(np.float32)
    ref_k, ref_i, _ = SM.pair_scan_ref(a, b, 5)
    kth2, idx, count = K.pair_scan(_dev(a, dev), _dev(b, dev), 5)
    assert count is None
    assert torch.isinf(kth2[:, 3:]).all() and (kth2[:, 3:] > 0).all() and (idx[:, 3:] == -1).all()
    assert np.array_equal(idx.cpu().numpy(), ref_i) and np.allclose(kth2[:, :3].cpu().numpy(), ref_k[:, :3], rtol=1e-5)
    kth2, idx, _ = K.pair_scan(_dev(b, dev), _dev(b, dev), 5, exclude_diag=True)           # Nb - 1 = 2 candidates
    assert torch.isinf(kth2[:, 2:]).all() and (idx[:, 2:] == -1).all() and (idx[:, :2] >= 0).all()
    assert np.array_equal(idx.cpu().numpy(), SM.pair_scan_ref(b, b, 5, exclude_diag=True)[1])


def test_pair_scan_duplicated_rows_tie_to_the_lower_index(dev):
    """b holds every row three times (j, j + 70, j + 140: two tiles of 128, so b is split in two and copies meet in the merge) and a is
    b's first rows.  A distance depends on the two rows' contents only, so copies tie EXACTLY -- at 0 up to the GEMM form's error, clamped
    at 0 from below -- and must come out lower index first; every further neighbour is such a triple too"""
    from dynamicvectorquantization_amd import kernels as K
    rng = np.random.default_rng(6)
    base = rng.normal(size=(70, 20)).astype(np.float32)
    b = np.concatenate([base, base, base], axis=0)                                          # 210 rows: copies at j, j + 70, j + 140
    a = base[:40]
    kth2, idx, _ = K.pair_scan(_dev(a, dev), _dev(b, dev), 6)
    kth2, idx = kth2.cpu().numpy(), idx.cpu().numpy()
    j = np.arange(40)
    assert np.array_equal(idx[:, :3], np.stack([j, j + 70, j + 140], axis=1))
    assert (kth2[:, 0] == kth2[:, 1]).all() and (kth2[:, 1] == kth2[:, 2]).all() and (kth2[:, 0] >= 0).all()
    assert (kth2[:, 0] <= SM.GRANTED * 2 * (a.astype(np.float64) ** 2).sum(axis=1)).all()
    ref_i = SM.pair_scan_ref(a, b, 6)[1]
    assert np.array_equal(idx[:, 3:] % 70, ref_i[:, 3:] % 70)                               # the next neighbour, three copies of it
    assert np.array_equal(idx[:, 3:], np.stack([idx[:, 3], idx[:, 3] + 70, idx[:, 3] + 140], axis=1)) and (idx[:, 3] < 70).all()
    assert (kth2[:, 3] == kth2[:, 4]).all() and (kth2[:, 4] == kth2[:, 5]).all() and (kth2[:, 3] > 0).all()


def test_pair_scan_padding_columns_are_never_read(dev):
    """lda / ldb > D with NaN in the padding columns: the same bits as the packed call.  D = 22 in pitch 24 takes the 16-byte loads up to
    column 20 and element loads behind; pitch 23 takes the element loads throughout"""
    from dynamicvectorquantization_amd import kernels as K
    c = scan_case(80, 96, 24, 3)
    a, b, rad = c["a"][:, :22], c["b"][:, :22], _dev(c["rad"], dev)
    want = K.pair_scan(_dev(a, dev), _dev(b, dev), 3, rad2_b=rad)
    for pitch in (24, 23):
        ap, bp = np.full((80, pitch), np.nan, np.float32), np.full((96, pitch), np.nan, np.float32)
        ap[:, :22], bp[:, :22] = a, b
        got = K.pair_scan(_dev(ap, dev)[:, :22], _dev(bp, dev)[:, :22], 3, rad2_b=rad)
        for w, g in zip(want, got):
            assert torch.equal(w, g), pitch


def test_pair_scan_without_radii_leaves_count_alone(dev):
    from dynamicvectorquantization_amd import kernels as K
    c = scan_case(64, 65, 7, 1)
    count = torch.full((64,), -7, dtype=torch.int64, device=dev)
    kth2, idx, out = K.pair_scan(_dev(c["a"], dev), _dev(c["b"], dev), 1, count=count)
    assert (count == -7).all()
    check_scan(c, 1, kth2, idx, None, label="no radii")


def test_pair_scan_k1_and_k16(dev):
    from dynamicvectorquantization_amd import kernels as K
    c = scan_case(257, 300, 1000, 5)
    a, b, rad = _dev(c["a"], dev), _dev(c["b"], dev), _dev(c["rad"], dev)
    k1, k16 = K.pair_scan(a, b, 1, rad2_b=rad), K.pair_scan(a, b, 16, rad2_b=rad)
    check_scan(c, 1, *k1, label="k = 1")
    check_scan(c, 16, *k16, label="k = 16")
    assert torch.equal(k1[0][:, 0], k16[0][:, 0]) and torch.equal(k1[1][:, 0], k16[1][:, 0]) and torch.equal(k1[2], k16[2])


def test_pair_scan_bad_arguments_launch_nothing(dev):
    from dynamicvectorquantization_amd import _lib
    lib = _lib.load()
    a, b = torch.zeros(20, 8, device=dev), torch.zeros(256, 8, device=dev)
    kth2 = torch.full((20, 16), -3.0, device=dev)
    idx = torch.full((20, 16), -3, dtype=torch.int64, device=dev)
    need = lib.dvq_pair_scan_workspace_bytes(20, 256, 2)
    assert need > 0
    ws = torch.zeros(need, dtype=torch.uint8, device=dev)
    p = lambda t: C.c_void_p(t.data_ptr())     # noqa: E731

    def call(k, d, ws_bytes, excl=0):
        return lib.dvq_pair_scan(p(a), 8, p(b), 8, 20, 256, d, None, k, excl, p(kth2), p(idx), None, p(ws), ws_bytes, None)

    assert call(0, 8, need) == -1 and call(17, 8, need) == -1 and call(2, 8, need, excl=2) == -1       # DVQ_EINVAL
    assert call(2, 0, need) == -2 and call(2, 9, need) == -2                                           # DVQ_ESHAPE (D = 0; D > pitch)
    assert call(2, 8, need - 1) == -5 and call(2, 8, 0) == -5                                          # DVQ_EWORKSPACE
    assert b"workspace" in lib.dvq_last_error()
    torch.cuda.synchronize()
    assert (kth2 == -3.0).all() and (idx == -3).all()
    assert call(2, 8, need) == 0
    torch.cuda.synchronize()
    got_d, got_i = kth2.view(-1)[:40].view(20, 2), idx.view(-1)[:40].view(20, 2)         # the outputs are [Na][k], packed
    assert (got_d == 0).all() and (got_i[:, 0] == 0).all() and (got_i[:, 1] == 1).all()
    assert (kth2.view(-1)[40:] == -3.0).all() and (idx.view(-1)[40:] == -3).all()


def test_pair_scan_is_reproducible_and_row_independent(dev):
    """two launches: equal bits.  a[:n1] and a[n1:] in two calls: the bits of one call -- with 8300 rows the whole call shares b's 17
    tiles out over 6 splits and the 100-row part over 9, and the second part's rows sit at other places of their tiles"""
    from dynamicvectorquantization_amd import _lib
    from dynamicvectorquantization_amd import kernels as K
    lib = _lib.load()
    real, fake = SM.make_sets(2100, 8300, 8, seed=11)
    xr, xf = SM.centre(real, fake)
    a, b = _dev(xf, dev), _dev(xr, dev)
    rad = K.pair_scan(b, b, 5, exclude_diag=True)[0][:, 4].contiguous()
    assert lib.dvq_pair_scan_workspace_bytes(8300, 2100, 5) // 8300 != lib.dvq_pair_scan_workspace_bytes(100, 2100, 5) // 100
    one = K.pair_scan(a, b, 5, rad2_b=rad)
    two = K.pair_scan(a, b, 5, rad2_b=rad)
    parts = [K.pair_scan(a[:100], b, 5, rad2_b=rad), K.pair_scan(a[100:], b, 5, rad2_b=rad)]
    for q in range(3):
        assert torch.equal(one[q], two[q])
        assert torch.equal(one[q], torch.cat([parts[0][q], parts[1][q]], dim=0))
    ref = SM.pair_scan_ref(xf[:64], xr, 5, rad2_b=rad.cpu().numpy())
    assert (one[1][:64].cpu().numpy() == ref[1]).mean() > 0.99


# ---- moments ------------------------------------------------------------------------------------------------------------------------
def moments_case(n, d, seed=0):
    real, _ = SM.make_sets(n, 8, d, seed=seed + n + d)
    x = real.astype(np.float32)
    shift = x[: min(n, 16)].mean(axis=0).astype(np.float32)
    return x, shift


def check_moments(got, x, shift):
    s, g, cnt = (t.cpu().numpy() for t in got)
    rs, rg, rn = SM.moments_ref(x, shift)
    assert int(cnt[0]) == rn
    assert (np.tril(g, -1) == 0).all(), "the lower triangle is the host's to mirror"
    fro = np.linalg.norm(rg)
    err_g = np.abs(g - np.triu(rg)).max() / fro
    y = np.abs((x - shift[None, :]).astype(np.float32).astype(np.float64))
    err_s = np.abs(s - rs).max() / y.sum(axis=0).max()
    print(f"moments {x.shape}: gram {err_g:.3e} of |G|_F, sum {err_s:.3e}")
    assert err_g <= 1e-12 and err_s <= 1e-12


@pytest.mark.parametrize("n,d", [(257, 24), (64, 7), (130, 1000), (33, 1024)], ids=lambda v: str(v))
def test_feat_moments_matches_fp64(dev, n, d):
    from dynamicvectorquantization_amd import kernels as K
    x, shift = moments_case(n, d)
    xd, sd = _dev(x, dev), _dev(shift, dev)
    got = K.feat_moments(xd, sd)
    check_moments(got, x, shift)
    again = K.feat_moments(xd, sd)
    for u, v in zip(got, again):
        assert torch.equal(u, v)


def test_feat_moments_streams_and_skips_padding(dev):
    from dynamicvectorquantization_amd import kernels as K
    x, shift = moments_case(257, 70)                     # 70 columns: a second tile of 6 columns
    sd = _dev(shift, dev)
    out = None
    for lo, hi in ((0, 100), (100, 101), (101, 257)):
        out = K.feat_moments(_dev(x[lo:hi], dev), sd, out=out)
    check_moments(out, x, shift)
    xp = np.full((257, 75), np.nan, np.float32)
    xp[:, :70] = x
    padded = K.feat_moments(_dev(xp, dev)[:, :70], sd)
    for u, v in zip(K.feat_moments(_dev(x, dev), sd), padded):
        assert torch.equal(u, v)


def test_feat_moments_bad_arguments(dev):
    from dynamicvectorquantization_amd import _lib
    lib = _lib.load()
    x, s, g, n = (torch.zeros(8, 4, device=dev), torch.zeros(4, dtype=torch.float64, device=dev),
                  torch.zeros(4, 4, dtype=torch.float64, device=dev), torch.zeros(1, dtype=torch.int64, device=dev))
    sh = torch.zeros(4, device=dev)
    p = lambda t: C.c_void_p(t.data_ptr())     # noqa: E731
    assert lib.dvq_feat_moments(p(x), 8, 0, 4, p(sh), p(s), p(g), p(n), None) == -2
    assert lib.dvq_feat_moments(p(x), 8, 4097, 4097, p(sh), p(s), p(g), p(n), None) == -2
    assert lib.dvq_feat_moments(p(x), 0, 4, 4, p(sh), p(s), p(g), p(n), None) == -2
    assert lib.dvq_feat_moments(p(x), 8, 4, 3, p(sh), p(s), p(g), p(n), None) == -2
    assert lib.dvq_feat_moments(None, 8, 4, 4, p(sh), p(s), p(g), p(n), None) == -1
    torch.cuda.synchronize()
    assert int(n[0]) == 0


# ---- the metrics end to end ------------------------------------------------------------------------------------------------------------
def test_sample_set_metrics_identity_and_disjoint(dev):
    from dynamicvectorquantization_amd import evaluate as E
    real, _ = SM.make_sets(257, 8, 40, seed=2)
    x = _dev(real, dev)
    ref, _, _ = SM.set_metrics_ref(real, real, 5)
    m = E.sample_set_metrics(x, x, k=5)
    assert m["precision"] == m["recall"] == m["coverage"] == 1.0
    assert m["density"] == pytest.approx(ref["density"], abs=1e-12)
    assert 0.0 <= m["fd"] <= 1e-9 * np.trace(SM.mean_cov(real)["cov"])
    assert (m["k"], m["n_real"], m["n_fake"], m["dim"]) == (5, 257, 257, 40)
    far = E.sample_set_metrics(x, x + 100.0, k=5)
    assert far["precision"] == far["recall"] == far["coverage"] == far["density"] == 0.0
    assert far["fd"] == pytest.approx(40 * 100.0 ** 2, rel=1e-6)


@pytest.mark.parametrize("na,nb,d,k", SM.PAIR_CASES, ids=lambda v: str(v))
def test_sample_set_metrics_match_the_restatement(dev, na, nb, d, k):
    """the five numbers against fp64, each within what the in-band pairs allow: a fake (real) row can change side only if one of its
    pairs is in the band, so precision (recall, coverage) may move by the in-band rows over the set size and density by the in-band pairs
    over k Nf -- computed per case by sampleset_math.set_metrics_ref and printed, 0 in most cases"""
    from dynamicvectorquantization_amd import evaluate as E
    c = scan_case(na, nb, d, k)
    ref, slack, frac = SM.set_metrics_ref(c["real"], c["fake"], k)
    m = E.sample_set_metrics(_dev(c["real"], dev), _dev(c["fake"], dev), k=k, neighbors=2)
    print(f"{(na, nb, d, k)}: allowed slack {slack}; in-band rows {frac}")
    assert frac["fr"] <= 0.02 and frac["rf"] <= 0.02
    for key in ("precision", "recall", "density", "coverage"):
        print(f"  {key}: {m[key]:.6f} (fp64 {ref[key]:.6f})")
        assert abs(m[key] - ref[key]) <= slack[key] + 1e-12, key
    # the moments are exact sums in another order: the Frechet term may move as far as the fp64 reference itself does under a change
    # of summation order (x 4), above a floor of 1e-9 tr S (the identity test's unit)
    tol = 4 * SM.fd_sensitivity(c["b"], c["a"]) + 1e-9 * np.trace(SM.mean_cov(c["b"])["cov"])
    print(f"  fd: {m['fd']:.12g} (fp64 {ref['fd']:.12g}), |difference| {abs(m['fd'] - ref['fd']):.3e}, allowed {tol:.3e}")
    assert abs(m["fd"] - ref["fd"]) <= tol
    assert (m["k"], m["n_real"], m["n_fake"], m["dim"]) == (k, nb, na, d)
    assert m["neighbor_idx"].shape == (na, 2) and (m["neighbor_idx"][:, 0] == c["idx"][:, 0]).mean() > 0.98


def test_sample_set_metrics_rejects_non_finite_rows(dev):
    from dynamicvectorquantization_amd import evaluate as E
    real, fake = SM.make_sets(40, 30, 6, seed=3)
    fake[4, 2] = np.inf
    with pytest.raises(ValueError, match="fake: 1 of 30"):
        E.sample_set_metrics(_dev(real, dev), _dev(fake, dev))
    with pytest.raises(ValueError, match="more than k rows"):
        E.sample_set_metrics(_dev(real, dev)[:5], _dev(real, dev), k=5)


# ---- the model path --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_pooled_features_and_evaluate_samples(dev, dtype):
    """the small golden DQ-VAE at its own image size, 2 synthetic batches of 8.  fp32: the features against an fp64 pooling of the
    quant_conv output taken from the model itself; the bound is the pooling's own rounding -- one x4 step on the 8 x 8 map sums 16 values
    and scales them, <= 17 roundings of 2^-24 relative to the largest |h|.  bf16: shape and finiteness only"""
    from dynamicvectorquantization_amd import dqvae
    from dynamicvectorquantization_amd import evaluate as E
    from dynamicvectorquantization_amd import runtime as rt
    from dynamicvectorquantization_amd import synth
    from dynamicvectorquantization_amd.config import instantiate_from_config
    from golden_cfg import dualformer_cfg
    with rt.compute_dtype_ctx(dtype):
        torch.manual_seed(0)
        model = instantiate_from_config(dualformer_cfg("uncond")["first_stage_config"]).to(dev)
        with torch.no_grad():
            for n, p in model.named_parameters():
                p.copy_(torch.from_numpy(synth.det_param(n, tuple(p.shape))).to(dev))
        rt.bump_weights_epoch()
        model.train()
        batches = [torch.from_numpy(synth.half_flat_images(8, 64, seed=s)).to(dev) for s in (31, 32)]
        f = model.pooled_features(batches[0], grid=2)
        assert model.training, "pooled_features leaves the mode as it found it"
        assert f.dtype == torch.float32 and tuple(f.shape) == (8, 64 * 4) and bool(torch.isfinite(f).all())
        assert tuple(model.pooled_features(batches[0], grid=1).shape) == (8, 64)
        with pytest.raises(ValueError):
            model.pooled_features(batches[0], grid=3)
        if dtype == "fp32":
            model.eval()
            with torch.no_grad():
                h = dqvae._merged_map(model, batches[0], None)[0]
            model.train()
            h = h[..., :64].double().cpu().numpy()                                       # NHWC [8, 8, 8, 64]
            want = h.reshape(8, 2, 4, 2, 4, 64).mean(axis=(2, 4)).reshape(8, -1)
            err = np.abs(f.cpu().numpy().astype(np.float64) - want).max()
            bound = 17 * 2.0 ** -24 * np.abs(h).max()
            print(f"pooled features vs fp64 pooling: {err:.3e}, bound {bound:.3e}")
            assert err <= bound
        s = E.evaluate_samples(model, batches, batches, k=5, grid=2, neighbors=1)
        assert s["precision"] == s["recall"] == s["coverage"] == 1.0
        assert (s["n_real"], s["n_fake"], s["dim"], s["grid"], s["features"], s["dtype"]) == (16, 16, 256, 2, "dqvae", dtype)
        feats = torch.cat([model.pooled_features(b, 2) for b in batches]).double().cpu().numpy()
        centred = SM.centre(feats, feats)[0].astype(np.float64)
        assert np.array_equal(s["neighbor_idx"][:, 0], np.arange(16))
        assert (s["neighbor_dist"][:, 0] <= SM.GRANTED * 2 * (centred ** 2).sum(axis=1)).all()
        assert 0.0 <= s["fd"] <= 1e-9 * np.trace(SM.mean_cov(feats)["cov"])
        assert "NOT the published FID" in s["note"] and "biased" in s["fd_note"]
