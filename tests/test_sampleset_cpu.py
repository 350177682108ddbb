"""CPU tests of the sample-set metrics (docs/design/32-sample-set-metrics.md): the numpy restatements against brute-force definitions,
the Frechet distance against scipy's matrix square root, the accuracy yardstick and the in-band caps of the GPU tests' shape matrix, the
non-finite-row rejection and scripts/tools/eval_samples.py up to the point where a GPU is needed."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import sampleset_math as SM
from conftest import REPO


def _script():
    spec = importlib.util.spec_from_file_location("eval_samples", os.path.join(REPO, "scripts", "tools", "eval_samples.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_library_and_build_know_the_new_kernels():
    from dynamicvectorquantization_amd import _lib, build
    assert "sampleset.hip" in build.SOURCES
    build.build(verbose=False)
    lib = _lib.load()
    for n in ("dvq_feat_moments", "dvq_pair_scan", "dvq_pair_scan_workspace_bytes"):
        assert n in _lib.SIGNATURES and hasattr(lib, n)
    # host-side argument checks run without a device: nothing is launched for any of these
    assert lib.dvq_pair_scan_workspace_bytes(80, 96, 3) == 0                        # one tile of b: not split, no workspace
    assert lib.dvq_pair_scan_workspace_bytes(20, 256, 2) == 2 * 20 * (2 * 8 + 8)    # two splits of (count, k distances, k indices) per row
    assert lib.dvq_pair_scan_workspace_bytes(20, 2100, 16) == 9 * 20 * (16 * 8 + 8)  # 17 tiles, two per split: 9 splits
    assert lib.dvq_pair_scan_workspace_bytes(80, 96, 0) == 0 and lib.dvq_pair_scan_workspace_bytes(80, 96, 17) == 0


def test_pair_scan_ref_against_loops():
    rng = np.random.default_rng(0)
    a, b = rng.normal(size=(9, 4)), rng.normal(size=(7, 4))
    rad = rng.uniform(1.0, 6.0, size=7)
    kth2, idx, count = SM.pair_scan_ref(a, b, 3, rad2_b=rad, exclude_diag=True)
    for i in range(9):
        cand = sorted((sum((a[i, c] - b[j, c]) ** 2 for c in range(4)), j) for j in range(7) if j != i)
        assert [j for _, j in cand[:3]] == list(idx[i])
        assert np.allclose([d for d, _ in cand[:3]], kth2[i], rtol=1e-14)
        assert count[i] == sum(1 for d, j in cand if d <= rad[j])
    # fewer candidates than k: +inf / -1 padding; duplicated rows: distance 0, the lower index first
    b2 = np.concatenate([b[:2], b[:1]])
    kth2, idx, _ = SM.pair_scan_ref(b2, b2, 5, exclude_diag=True)
    assert np.isinf(kth2[:, 2:]).all() and (idx[:, 2:] == -1).all()
    assert kth2[0, 0] == 0.0 and idx[0, 0] == 2 and idx[2, 0] == 0
    kth2, idx, _ = SM.pair_scan_ref(b2, b2, 2)
    assert list(idx[0]) == [0, 2] and list(idx[2]) == [0, 2]


def test_set_metrics_ref_against_definitions():
    """precision / recall (Kynkaanniemi et al. 2019) and density / coverage (Naeem et al. 2020) written out with loops"""
    real, fake = SM.make_sets(30, 26, 5, seed=1)
    k = 3
    m, slack, _ = SM.set_metrics_ref(real, fake, k)
    xr, xf = SM.centre(real, fake)
    xr, xf = xr.astype(np.float64), xf.astype(np.float64)
    dist = lambda u, v: float(((u - v) ** 2).sum())     # noqa: E731
    rad_r = [sorted(dist(xr[i], xr[j]) for j in range(30) if j != i)[k - 1] for i in range(30)]
    rad_f = [sorted(dist(xf[i], xf[j]) for j in range(26) if j != i)[k - 1] for i in range(26)]
    prec = np.mean([any(dist(f, xr[j]) <= rad_r[j] for j in range(30)) for f in xf])
    rec = np.mean([any(dist(r, xf[j]) <= rad_f[j] for j in range(26)) for r in xr])
    dens = sum(sum(dist(f, xr[j]) <= rad_r[j] for j in range(30)) for f in xf) / (k * 26)
    cov = np.mean([min(dist(xr[i], f) for f in xf) <= rad_r[i] for i in range(30)])
    assert (m["precision"], m["recall"], m["density"], m["coverage"]) == pytest.approx((prec, rec, dens, cov), abs=1e-15)
    assert 0 < m["precision"] < 1 or 0 < m["recall"] < 1                 # the recipe is not degenerate
    assert all(v >= 0 for v in slack.values())
    same, _, _ = SM.set_metrics_ref(real, real, k)
    assert same["precision"] == same["recall"] == same["coverage"] == 1.0 and same["fd"] <= 1e-9 * np.trace(SM.mean_cov(real)["cov"])
    far, _, _ = SM.set_metrics_ref(real, real + 100.0, k)
    assert far["precision"] == far["recall"] == far["coverage"] == far["density"] == 0.0


def test_frechet_distance_against_sqrtm():
    from scipy.linalg import sqrtm

    from dynamicvectorquantization_amd import evaluate as E
    for n_r, n_f, d, seed in [(200, 180, 16, 0), (300, 320, 64, 1), (150, 150, 7, 2)]:
        real, fake = SM.make_sets(n_r, n_f, d, seed)
        mr, mf = SM.mean_cov(real), SM.mean_cov(fake)
        root = sqrtm(mr["cov"] @ mf["cov"])
        dm = mr["mean"] - mf["mean"]
        ref = float(dm @ dm + np.trace(mr["cov"]) + np.trace(mf["cov"]) - 2.0 * np.trace(root).real)
        got = E.frechet_distance(mr, mf)
        assert got == pytest.approx(ref, rel=1e-6), (n_r, n_f, d)
        assert got == pytest.approx(SM.frechet_eigh(mr, mf), rel=1e-12)
    # rank-deficient: 40 and 50 rows in 64 dimensions
    real, fake = SM.make_sets(40, 50, 64, 3)
    fd = E.frechet_distance(SM.mean_cov(real), SM.mean_cov(fake))
    assert np.isfinite(fd) and fd >= 0.0
    assert E.frechet_distance(SM.mean_cov(real), SM.mean_cov(real)) <= 1e-9 * np.trace(SM.mean_cov(real)["cov"])


def test_moments_from_sums_mirrors_and_divides_by_n_minus_1():
    from dynamicvectorquantization_amd import evaluate as E
    rng = np.random.default_rng(4)
    x = rng.normal(size=(50, 6)).astype(np.float32)
    shift = rng.normal(size=6).astype(np.float32)
    s, g, n = SM.moments_ref(x, shift)
    m = E.moments_from_sums(s, np.triu(g), np.array([n]), shift)         # the kernel writes the upper triangle only
    y = (x - shift[None, :]).astype(np.float64)
    assert np.allclose(m["mean"], y.mean(axis=0) + shift, rtol=0, atol=1e-12)
    assert np.allclose(m["cov"], np.cov(y, rowvar=False, ddof=1), rtol=0, atol=1e-12) and m["n"] == 50
    with pytest.raises(ValueError):
        E.moments_from_sums(s, g, np.array([1]))


def test_staging_yardstick_and_band():
    """the accuracy bound of the GPU tests comes from here: the numpy float32 restatement of the kernel's staging against fp64 on the
    shape matrix, in units of |a|^2 + |b|^2; the GPU is granted 4 x that, and the decision band must be at least twice the grant"""
    worst = 0.0
    for na, nb, d, k in SM.PAIR_CASES + SM.PAIR_EDGE_CASES:
        xr, xf = SM.centre(*SM.make_sets(nb, na, d, seed=SM.case_seed(na, nb, d)))
        worst = max(worst, SM.staging_error(xf, xr), SM.staging_error(xr, xr))
    print(f"fp32 staging vs fp64: worst {worst:.3e} of (|a|^2 + |b|^2); recorded yardstick {SM.STAGING_YARDSTICK:.3e}, "
          f"granted {SM.GRANTED:.3e}, band {SM.BAND:.1e}")
    assert worst <= SM.STAGING_YARDSTICK <= 1.25 * worst          # the recorded value is the measured one, rounded up
    assert SM.GRANTED == 4 * SM.STAGING_YARDSTICK and SM.BAND >= 2 * SM.GRANTED


@pytest.mark.parametrize("na,nb,d,k", SM.PAIR_CASES + SM.PAIR_EDGE_CASES, ids=lambda v: str(v))
def test_in_band_rows_stay_under_the_cap(na, nb, d, k):
    """a GPU test that excludes too many rows checks nothing: rows with any in-band pair stay <= 2 % in every case, for the count
    decisions of the F|R scan (radii given) and for the end-to-end metrics (radii computed)"""
    real, fake = SM.make_sets(nb, na, d, seed=SM.case_seed(na, nb, d))
    xr, xf = SM.centre(real, fake)
    rad = SM.pair_scan_ref(xr, xr, min(k, nb - 1), exclude_diag=True)[0][:, min(k, nb - 1) - 1].astype(np.float32)
    rows = SM.in_band(SM.d2_fp64(xf, xr), rad, SM.norm_scale(xf, xr)).any(axis=1).mean()
    m, slack, frac = SM.set_metrics_ref(real, fake, min(k, min(na, nb) - 1))
    print(f"in-band rows: scan {rows:.4f}, end to end F|R {frac['fr']:.4f} R|F {frac['rf']:.4f}; slack {slack}")
    assert rows <= 0.02 and frac["fr"] <= 0.02 and frac["rf"] <= 0.02


def test_non_finite_rows_are_rejected():
    from dynamicvectorquantization_amd import evaluate as E
    x = torch.zeros(20, 4)
    y = x.clone()
    y[3, 1] = float("nan")
    y[7, 0] = float("inf")
    y[7, 2] = float("nan")
    with pytest.raises(ValueError, match="fake: 2 of 20"):
        E.sample_set_metrics(x, y)
    with pytest.raises(ValueError, match="real: 2 of 20"):
        E.sample_set_metrics(y, x)
    with pytest.raises(TypeError):
        E.sample_set_metrics(x.long(), x)


def test_script_arguments_and_json_keys(tmp_path):
    ES = _script()
    real, fake = SM.make_sets(12, 10, 5, seed=0)
    np.save(tmp_path / "r.npy", real.astype(np.float32))
    np.save(tmp_path / "f.npy", fake)
    opt = ES.parse_args(["--features", "npy", "--real", str(tmp_path / "r.npy"), "--fake", str(tmp_path / "f.npy"), "--k", "3",
                         "--limit", "8", "--neighbors", "2", "--neighbors_out", str(tmp_path / "nn.npz")])
    assert (opt.features, opt.k, opt.limit, opt.neighbors, opt.grid) == ("npy", 3, 8, 2, 2)
    a = ES.load_features(opt.real, opt.limit)
    assert a.shape == (8, 5) and ES.load_features(opt.fake).shape == (10, 5)
    m, _, _ = SM.set_metrics_ref(real[:8], fake[:8], 3)
    line = ES.record(opt, m)
    assert set(ES.KEYS) <= set(line) and line["features"] == "npy" and line["neighbors"] == 2
    assert "published" in line["note"] and "biased" in line["fd_note"]
    dq = ES.parse_args(["--real", "a", "--fake", "b.npz", "--yaml_path", "c.yml", "--use_ema"])
    line = ES.record(dq, dict(m, grid=2, dtype="bf16"))
    assert line["features"] == "dqvae" and "NOT the published FID" in line["note"] and line["grid"] == 2 and line["use_ema"] is True
    for bad in (["--real", "a", "--fake", "b"],                                                        # dqvae needs a YAML
                ["--features", "npy", "--real", "a.npy", "--fake", "b.npz"],                           # npy features from .npy only
                ["--features", "npy", "--real", "a.npy", "--fake", "b.npy", "--k", "17"],
                ["--features", "npy", "--real", "a.npy", "--fake", "b.npy", "--neighbors", "2"]):      # no --neighbors_out
        with pytest.raises(SystemExit):
            ES.parse_args(bad)
    np.save(tmp_path / "bad.npy", np.zeros((3, 4, 5), np.float32))
    with pytest.raises(ValueError):
        ES.load_features(str(tmp_path / "bad.npy"))
    np.savez(tmp_path / "s.npz", np.full((5, 8, 8, 3), 255, np.uint8))
    xs = list(ES.npz_batches(str(tmp_path / "s.npz"), 2, 8, "cpu", limit=3))
    assert [tuple(x.shape) for x in xs] == [(2, 3, 8, 8), (1, 3, 8, 8)] and float(xs[0].max()) == 1.0
    with pytest.raises(ValueError):
        list(ES.npz_batches(str(tmp_path / "s.npz"), 2, 16, "cpu"))
