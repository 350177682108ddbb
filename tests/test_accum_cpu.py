"""Gradient accumulation, host side (docs/design/28-gradient-accumulation.md): the window-boundary rule, the optimizer-step arithmetic, the
learning-rate rule with the reference's factor, and tests/accum_math.py -- Adam over windows against torch.optim, and the windowed
two-optimizer schedule around oracle.train_step against the reference fixture tests/golden/train_step_accum_small.npz."""
import pytest
import torch

from conftest import load_golden


# ---- the host arithmetic of windows -------------------------------------------------------------------------------------------------------
def _closing_batches(n, k, bpe):
    from dynamicvectorquantization_amd.trainer import window_schedule
    return [b + 1 for b, (_, last) in enumerate(window_schedule(n, k, bpe)) if last]


def test_window_boundaries():
    """a window closes when (batch_in_epoch + 1) % k == 0 or with the epoch's last batch; 1-based batch numbers after which a step falls"""
    from dynamicvectorquantization_amd.trainer import window_flags, window_schedule
    assert _closing_batches(8, 2, 4) == [2, 4, 6, 8]
    assert _closing_batches(7, 2, 3) == [2, 3, 5, 6]
    assert _closing_batches(10, 3, 5) == [3, 5, 8, 10]
    assert _closing_batches(4, 4, 1) == [1, 2, 3, 4]
    assert _closing_batches(10, 3, None) == [3, 6, 9]
    for bpe, k in ((4, 2), (3, 2), (5, 3), (1, 4), (None, 3)):
        sched = window_schedule(23, k, bpe)
        assert sched[0][0]                                                     # a run opens a window
        for (_, last), (first, _) in zip(sched, sched[1:]):
            assert first == last                                               # a window opens exactly where one closed
        for b, (first, last) in enumerate(sched):
            bie = b % bpe if bpe else b
            assert last == ((bie + 1) % k == 0 or (bpe is not None and bie + 1 == bpe)), (bpe, k, b)
            assert first == (bie % k == 0), (bpe, k, b)
    assert window_flags(0, 0, 1) == (True, True)


def test_optimizer_steps_per_epoch_is_the_ceiling():
    from dynamicvectorquantization_amd.trainer import optimizer_steps_per_epoch
    for bpe in (1, 2, 3, 4, 5, 100, 1281):
        for k in (1, 2, 3, 4, 8):
            want = len(_closing_batches(bpe, k, bpe))
            assert optimizer_steps_per_epoch(bpe, k) == want == (bpe + k - 1) // k, (bpe, k)


def test_learning_rate_rule_takes_the_factor():
    from dynamicvectorquantization_amd.trainer import reference_learning_rate
    cfg = {"base_learning_rate": 4.5e-6}
    assert reference_learning_rate(cfg, 2, 30) == 2 * 30 * 4.5e-6              # as ever
    assert reference_learning_rate(cfg, 2, 30, 1) == reference_learning_rate(cfg, 2, 30)
    assert reference_learning_rate(cfg, 2, 30, 4) == 4 * 2 * 30 * 4.5e-6       # train.py:255 of the reference
    assert reference_learning_rate({"learning_rate": 1e-3}, 8, 64, 4) == 1e-3  # an absolute rate is nobody's to scale
    with pytest.raises(NotImplementedError):
        reference_learning_rate({}, 1, 1, 2)


@pytest.mark.parametrize("kind", ["adam", "adamw"])
def test_accum_math_adam_over_windows_matches_torch_optim(kind):
    """tests/accum_math.py (fp64 Adam on the fp32-accumulated window gradient) against torch.optim fed the same sums: k = 3, four
    windows, the last one short (two micro-batches, still divided by 3), a learning rate that changes every window.  Both sides see
    identical fp32 gradients; fp64 against torch's fp32 update: 3e-6, the bound of the HipAdam-versus-torch tests"""
    import numpy as np
    from accum_math import AdamOverWindows, accumulate
    rs = np.random.RandomState(3)
    k, shape = 3, (37, 5)
    betas, wd = ((0.5, 0.9), 0.0) if kind == "adam" else ((0.9, 0.95), 0.01)
    p0 = rs.standard_normal(shape).astype(np.float32)
    q = torch.nn.Parameter(torch.from_numpy(p0.copy()))
    ref = (torch.optim.Adam if kind == "adam" else torch.optim.AdamW)([q], lr=1e-3, betas=betas, weight_decay=wd)
    mine = AdamOverWindows(p0, 1e-3, betas, weight_decay=wd)
    for t, n_micro in enumerate((3, 3, 3, 2)):
        lr = 1e-3 * (0.5 + 0.25 * t)
        ref.param_groups[0]["lr"], mine.lr = lr, lr
        micro = [rs.standard_normal(shape).astype(np.float32) * np.float32(10.0 ** rs.randint(-4, 2)) for _ in range(n_micro)]
        q.grad = torch.from_numpy(accumulate(micro, k))
        ref.step()
        g = mine.step(micro, k)
        assert np.array_equal(g.astype(np.float32), q.grad.numpy())
        if n_micro < k:                                                        # the short window: sum / k, not the mean
            # fl(1/3), two rounded products and one rounded addition: at most four roundings of 2^-24 of the summed magnitudes
            exact = sum(m.astype(np.float64) for m in micro) / k
            assert np.all(np.abs(g - exact) <= 4 * 2.0 ** -24 * sum(np.abs(m.astype(np.float64)) for m in micro) / k)
        np.testing.assert_allclose(mine.p, q.detach().numpy(), rtol=3e-6, atol=1e-9)
    ea = ref.state[q]["exp_avg"].numpy()             # signed sums cancel: the absolute floor of test_hip_adam_matches_torch_optim
    np.testing.assert_allclose(mine.m, ea, rtol=3e-6, atol=1e-6 * float(np.abs(ea).max()))
    np.testing.assert_allclose(mine.v, ref.state[q]["exp_avg_sq"].numpy(), rtol=3e-6, atol=1e-30)


def test_windowed_schedule_matches_the_reference_fixture():
    """tests/accum_math.py::accum_schedule_steps (oracle.train_step's ae_forward, Adam and adam_update inside Lightning's window: zero on
    the first micro-batch, loss / k backwards, step on the closing one) against the reference's own run of the same six micro-batches
    (tools/gen_golden_accum.py): k = 2, window 0 at lr 0, window 1 at the full rate, window 2 the first of a second epoch.  Same
    distances and the same bounds as the one-step pin (compare_records / check_summary, PIN_BOUNDS), which includes zero code rows
    differing at gaps >= 1e-4 before the first real update and parameters exactly unmoved by the lr = 0 window."""
    import accum_math as A
    from dynamicvectorquantization_amd import synth
    from oracle import train_step as ots
    g = load_golden("train_step_accum_small")
    ref = {k_: g[k_] for k_ in g.files}
    meta = {k_: g[k_] for k_ in ("state_keys", "state_shapes", "param_keys")}
    got = A.accum_schedule_steps(meta)
    missing = [k_ for k_ in ref if k_ not in got and not k_.startswith(("state_", "param_keys"))]
    assert not missing, missing
    # what the fixture holds, where: rates and accumulated gradients on closing micro-batches only
    closing = sorted(int(k_.split(".")[0][1:]) for k_ in ref if k_.endswith(".o0.lr"))
    assert closing == [1, 3, 5] and float(ref["s1.o0.lr"]) == 0.0 and float(ref["s3.o0.lr"]) == 2e-5 and 0 < float(ref["s5.o0.lr"]) < 2e-5
    assert sorted({k_.split(".")[0] for k_ in ref if ".grad." in k_ or ".exp_avg." in k_}) == ["s1", "s3", "s5"]
    assert all(f"s{b}.o{i}.codes" in ref and f"s{b}.o{i}.cluster_size_ema" in ref for b in range(6) for i in (0, 1))
    geom = synth.DQVAE_GEOM["small"]
    cmp = ots.compare_records(got, ref, start_param=ots.sampled_start_param(meta, geom["k"], geom["zc"], A.accum_stride))
    summ = ots.summarize(cmp)
    assert ("s1", "dparam0") in summ and ("s3", "dparam") in summ and ("s5", "grad_disc") in summ
    bad = ots.check_summary(summ)
    assert not bad, bad
