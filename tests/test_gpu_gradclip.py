"""Global-norm gradient clipping and the non-finite step guard (docs/design/19-gradient-clipping.md): dvq_grad_sqnorm against fp64,
dvq_adamw_clip_dev through HipAdam.set_grad_guard against torch.optim on the CPU, and the Trainer's eager / recorded / checkpoint paths.
`pytest -m gpu`."""
import numpy as np
import pytest
import torch

from dynamicvectorquantization_amd import synth

pytestmark = pytest.mark.gpu

SHAPES = [(37, 5), (1,), (8, 4, 3, 3), (11,), (6, 6), (130, 7)]      # of test_hip_adam_matches_torch_optim, restated
WD = 0.01


def _chunk():
    from dynamicvectorquantization_amd import kernels as K
    c = K.GRAD_SQNORM_CHUNK
    assert K.grad_sqnorm_workspace_bytes(c) == 8 and K.grad_sqnorm_workspace_bytes(c + 1) == 16      # the library's own chunk length
    return c


def _scaled_normal(rs, n):
    """N(0,1) times per-block scales 1e-6 .. 1e2 (blocks of ~n/7 elements)"""
    x = rs.standard_normal(n).astype(np.float32)
    edges = np.linspace(0, n, 8).astype(np.int64)
    for a, b in zip(edges[:-1], edges[1:]):
        x[a:b] *= np.float32(10.0 ** rs.randint(-6, 3))
    return x


def _stats(dev, x, clip=0.0, skip=False, gstat=None):
    from dynamicvectorquantization_amd import kernels as K
    g = torch.from_numpy(x).to(dev)
    ws = torch.empty(K.grad_sqnorm_workspace_bytes(g.numel()) // 8, dtype=torch.float64, device=dev)
    gstat = K.grad_stats_block(dev) if gstat is None else gstat
    K.grad_sqnorm(g, ws, gstat, clip, skip)
    return K.read_grad_stats(gstat), gstat.cpu().numpy().copy()


def test_norm_matches_fp64(dev):
    """sizes around the chunk length and the 16-byte vector; only the ORDER of the fp64 additions differs from numpy's (the squares
    of fp32 values are exact in fp64): relative bound n * 2^-53 * 4.  Same buffer twice: bit-equal statistics."""
    c = _chunk()
    rs = np.random.RandomState(11)
    for n in (1, 3, c - 1, c, c + 1, 3 * c + 5):
        x = _scaled_normal(rs, n)
        want = float(np.linalg.norm(x.astype(np.float64)))
        clip = want / 3.0
        st, raw = _stats(dev, x, clip=clip)
        err = abs(st["norm"] - want) / want
        print(f"n={n}: norm {st['norm']:.17g} fp64 {want:.17g} rel err {err:.3g} bound {n * 2.0 ** -53 * 4:.3g}")
        assert err <= n * 2.0 ** -53 * 4, n
        assert st["finite"] and st["skipped"] == 0
        want_coef = np.float32(min(1.0, float(np.float32(clip)) / (want + 1e-6)))
        assert abs(np.float32(st["coef"]) - want_coef) <= np.spacing(want_coef), n
        st2, raw2 = _stats(dev, x, clip=clip)
        assert np.array_equal(raw, raw2), n                                  # norm, coef, flags: bit for bit
    st, _ = _stats(dev, np.zeros(c + 9, np.float32), clip=1.0)
    assert st["norm"] == 0.0 and st["coef"] == 1.0 and st["finite"]


def test_finite_flag_has_no_false_alarms_and_no_misses(dev):
    c = _chunk()
    rs = np.random.RandomState(12)
    n = c + 7                                                                # n % 4 == 3: the last elements take the scalar tail
    base = rs.standard_normal(n).astype(np.float32)
    big = base.copy()
    big[[0, 5, c // 2, c + 1, n - 1]] = np.float32(1e25) * np.array([1, -1, 1, -1, 1], np.float32)
    with np.errstate(over="ignore"):
        assert not np.isfinite(np.float32(1e25) * np.float32(1e25))          # the fp32 square overflows ...
    want = float(np.linalg.norm(big.astype(np.float64)))
    st, _ = _stats(dev, big, clip=1.0, skip=True)
    assert st["finite"] and st["skipped"] == 0                               # ... the fp64 one does not
    assert abs(st["norm"] - want) / want <= n * 2.0 ** -53 * 4
    for pos, val in ((n - 1, np.nan), (n // 2, np.inf), (0, -np.inf)):
        bad = base.copy()
        bad[pos] = val
        st, _ = _stats(dev, bad, clip=1.0, skip=True)
        assert not st["finite"] and st["skipped"] == 1, (pos, val, st)
        st, _ = _stats(dev, bad, clip=0.0, skip=False)
        assert not st["finite"] and st["skipped"] == 0 and st["coef"] == 1.0, (pos, val, st)


# ---- HipAdam with the guard against torch.optim on the CPU -----------------------------------------------------------------------
def _optimizers(dev, kind, p0, guard=None):
    from dynamicvectorquantization_amd.trainer import HipAdam
    betas = (0.5, 0.9) if kind == "adam" else (0.9, 0.95)
    ref_p = [torch.nn.Parameter(torch.from_numpy(a.copy())) for a in p0]
    hip_p = [torch.nn.Parameter(torch.from_numpy(a.copy()).to(dev)) for a in p0]
    if kind == "adam":
        ref_opt = torch.optim.Adam(ref_p, lr=1e-3, betas=betas)
        hip_opt = HipAdam(hip_p, lr=1e-3, betas=betas)
    else:
        ref_opt = torch.optim.AdamW([{"params": ref_p[:3], "weight_decay": WD}, {"params": ref_p[3:], "weight_decay": 0.0}], lr=1e-3, betas=betas)
        hip_opt = HipAdam([{"params": hip_p[:3], "weight_decay": WD}, {"params": hip_p[3:], "weight_decay": 0.0}], lr=1e-3, betas=betas)
    hip_opt.flatten()
    if guard is not None:
        hip_opt.set_grad_guard(*guard)
    return ref_p, ref_opt, hip_p, hip_opt


def _draw(rs):
    p0 = [rs.standard_normal(s).astype(np.float32) * (1e-3 if i == 3 else 1.0) for i, s in enumerate(SHAPES)]
    steps = []
    for _ in range(4):
        grads = [rs.standard_normal(s).astype(np.float32) * (10.0 ** rs.randint(-6, 2)) for s in SHAPES]
        grads[4][:] = 0.0                                                    # a tensor whose gradient is exactly zero
        steps.append(grads)
    return p0, steps


def _norm64(grads):
    return float(np.linalg.norm(np.concatenate([g.ravel().astype(np.float64) for g in grads])))


def _set_lr(opts, t):
    for opt in opts:
        for grp in opt.param_groups:
            grp["lr"] = 1e-3 * (0.5 + 0.25 * t)                              # a learning rate that changes every step


def _load_grads(dev, ref_p, hip_p, grads, scale=None):
    for q, h, gq in zip(ref_p, hip_p, grads):
        q.grad = torch.from_numpy(gq.copy() if scale is None else gq * scale)        # fp32 * fp32 scalar: rounded in fp32
        h.grad.copy_(torch.from_numpy(gq).to(dev))


def _assert_params(ref_p, hip_p, msg):
    for i, (q, h) in enumerate(zip(ref_p, hip_p)):
        np.testing.assert_allclose(h.detach().cpu().numpy(), q.detach().numpy(), rtol=3e-6, atol=1e-9, err_msg=f"{msg} tensor {i}")


def _assert_moments(ref_p, ref_opt, hip_p, hip_opt):
    from dynamicvectorquantization_amd.trainer import FlatParams
    m, v = hip_opt._fstate["m"], hip_opt._fstate["v"]
    off = 0
    for q, h in zip(ref_p, hip_p):
        ea = ref_opt.state[q]["exp_avg"].numpy()
        ev = ref_opt.state[q]["exp_avg_sq"].numpy()
        np.testing.assert_allclose(FlatParams._view(m, off, h).cpu().numpy(), ea, rtol=3e-6, atol=1e-6 * max(1e-30, float(np.abs(ea).max())))
        np.testing.assert_allclose(FlatParams._view(v, off, h).cpu().numpy(), ev, rtol=3e-6, atol=1e-30)
        off += h.numel()


@pytest.mark.parametrize("kind", ["adam", "adamw"])
def test_clipped_adam_matches_torch_optim(dev, kind):
    """reference per step: coef32 = float32(min(1, clip / (norm64 + 1e-6))), gradients * coef32 in fp32, torch's own step(); bounds of
    test_hip_adam_matches_torch_optim.  The clip value sits between the smallest and the largest of the four gradient norms."""
    p0, steps = _draw(np.random.RandomState(1))
    norms = [_norm64(g) for g in steps]
    clip = float(np.float32(np.sqrt(min(norms) * max(norms))))
    ref_p, ref_opt, hip_p, hip_opt = _optimizers(dev, kind, p0, guard=(clip, False))
    coefs = []
    for t, grads in enumerate(steps, start=1):
        _set_lr((ref_opt, hip_opt), t)
        coef32 = np.float32(min(1.0, clip / (norms[t - 1] + 1e-6)))
        coefs.append(float(coef32))
        _load_grads(dev, ref_p, hip_p, grads, scale=coef32)
        g_before = hip_opt.flat.flat_g.clone()
        ref_opt.step()
        hip_opt.step()
        st = hip_opt.grad_stats()
        assert abs(np.float32(st["coef"]) - coef32) <= np.spacing(coef32), (t, st, coef32)
        assert st["finite"] and st["skipped"] == 0
        assert torch.equal(hip_opt.flat.flat_g, g_before)                    # the gradient buffer is read, never rewritten
        _assert_params(ref_p, hip_p, f"{kind} t={t}")
    assert min(coefs) < 0.5 and max(coefs) == 1.0, coefs                      # one step clipped hard, one not at all
    _assert_moments(ref_p, ref_opt, hip_p, hip_opt)


def test_guard_only_is_bit_identical_on_finite_gradients(dev):
    p0, steps = _draw(np.random.RandomState(2))
    _, _, plain_p, plain = _optimizers(dev, "adamw", p0)
    _, _, guard_p, guard = _optimizers(dev, "adamw", p0, guard=(0.0, True))
    for t, grads in enumerate(steps[:3], start=1):
        _set_lr((plain, guard), t)
        for a, b, gq in zip(plain_p, guard_p, grads):
            a.grad.copy_(torch.from_numpy(gq).to(dev))
            b.grad.copy_(torch.from_numpy(gq).to(dev))
        plain.step()
        guard.step()
    assert torch.equal(plain.flat.flat_p, guard.flat.flat_p)
    assert torch.equal(plain._fstate["m"], guard._fstate["m"]) and torch.equal(plain._fstate["v"], guard._fstate["v"])
    st = guard.grad_stats()
    assert st["skipped"] == 0 and st["coef"] == 1.0 and st["finite"]
    assert plain.grad_stats() is None


def test_nonfinite_step_is_skipped(dev):
    """steps 1, 2 finite, step 3 with one NaN, step 4 finite.  The skipped step leaves p, m, v bit for bit and still advances the step
    count; the torch reference skips its step() there and advances every state["step"] by hand."""
    p0, steps = _draw(np.random.RandomState(3))
    steps[2][5][17, 3] = np.nan
    ref_p, ref_opt, hip_p, hip_opt = _optimizers(dev, "adamw", p0, guard=(0.0, True))
    _, _, bare_p, bare = _optimizers(dev, "adamw", p0)                        # the same input without the guard
    for t, grads in enumerate(steps, start=1):
        _set_lr((ref_opt, hip_opt, bare), t)
        _load_grads(dev, ref_p, hip_p, grads)
        for b, gq in zip(bare_p, grads):
            b.grad.copy_(torch.from_numpy(gq).to(dev))
        before = [x.clone() for x in (hip_opt.flat.flat_p, hip_opt._fstate["m"], hip_opt._fstate["v"])]
        hip_opt.step()
        bare.step()
        if t == 3:
            for q in ref_p:
                ref_opt.state[q]["step"] += 1
            for a, b in zip(before, (hip_opt.flat.flat_p, hip_opt._fstate["m"], hip_opt._fstate["v"])):
                assert torch.equal(a, b)
            st = hip_opt.grad_stats()
            assert st["skipped"] == 1 and not st["finite"] and hip_opt._fstate["step"] == 3
        else:
            ref_opt.step()
            assert hip_opt.grad_stats()["finite"]
    assert hip_opt.grad_stats()["skipped"] == 1
    _assert_params(ref_p, hip_p, "after the skipped step")
    _assert_moments(ref_p, ref_opt, hip_p, hip_opt)
    assert bool(torch.isnan(bare.flat.flat_p).any())                         # the case is real: unguarded, the NaN reaches the parameters


def test_argument_checks(dev):
    from dynamicvectorquantization_amd.trainer import HipAdam
    ps = [torch.nn.Parameter(torch.zeros(5, device=dev))]
    opt = HipAdam(ps)
    with pytest.raises(ValueError, match="flatten"):
        opt.set_grad_guard(1.0)
    opt.flatten()
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            opt.set_grad_guard(bad)
    opt.set_grad_guard(1.0, True)
    assert opt.grad_stats() == {"norm": 0.0, "coef": 1.0, "finite": True, "skipped": 0}


# ---- Trainer -------------------------------------------------------------------------------------------------------------------
def _make(dev, use_graph, graph_after=2, seed=0, **guard):
    """tests/test_gpu_stepgraph.py::_make with the `ae` objective, plus the guard arguments"""
    from dynamicvectorquantization_amd.config import instantiate_from_config
    from dynamicvectorquantization_amd.trainer import Trainer
    from test_gpu_model import GEOM, model_config
    torch.manual_seed(seed)
    model = instantiate_from_config(model_config(**GEOM["small"], loss="ae")).to(dev)
    model.learning_rate, model.min_learning_rate = 2e-4, 1e-5
    model.training_steps, model.steps_per_epoch, model.warmup_epochs = 12, 4, 1
    model.train()
    return model, Trainer(model, max_steps=12, use_graph=use_graph, graph_after=graph_after, **guard)


def _images(dev):
    return [torch.from_numpy(synth.half_flat_images(2, 64, seed=40 + i)).to(dev) for i in range(3)]


@pytest.fixture(scope="module")
def unclipped(dev):
    """one eager step with the norm measured but nothing clipped -> (norm0, Adam first moments)"""
    from dynamicvectorquantization_amd import runtime as rt
    with rt.compute_dtype_ctx(torch.float32):
        model, tr = _make(dev, False, skip_nonfinite=True)
        assert len(tr.opts) == 1
        tr.train_step({"image": _images(dev)[0]}, 0)
        st = tr.grad_stats()[0]
        assert st["finite"] and st["coef"] == 1.0 and st["norm"] > 0
        return st["norm"], tr.opts[0]._fstate["m"].clone()


def test_trainer_eager_clips(dev, unclipped):
    """clip at a quarter of the measured norm: coef = 0.25 and, Adam's first update being invariant to a gradient rescale, the first
    moments (not the parameters) show it; 2e-3 is the run-to-run bound of test_step_graph_matches_eager for this objective"""
    from dynamicvectorquantization_amd import runtime as rt
    norm0, m0 = unclipped
    with rt.compute_dtype_ctx(torch.float32):
        model, tr = _make(dev, False, gradient_clip_val=norm0 / 4)
        tr.train_step({"image": _images(dev)[0]}, 0)
        st = tr.grad_stats()[0]
    print(f"norm0 {norm0:.6g} clipped run: {st}")
    assert abs(st["coef"] - 0.25) <= 2e-3 * 0.25
    want = st["coef"] * m0
    assert float((tr.opts[0]._fstate["m"] - want).norm()) <= 2e-3 * float(want.norm())


def test_trainer_recorded_step_clips(dev, unclipped):
    from dynamicvectorquantization_amd import runtime as rt
    norm0, _ = unclipped
    xs, steps = _images(dev), 8
    runs = []
    with rt.compute_dtype_ctx(torch.float32):
        for use_graph in (False, True):
            model, tr = _make(dev, use_graph, gradient_clip_val=norm0 / 4, skip_nonfinite=True)
            losses, stats = [], []
            for i in range(steps):
                out = tr.train_step({"image": xs[i % 3]}, i)
                losses.append([float(l) for l in out])
                stats.append(tr.grad_stats()[0])
            torch.cuda.synchronize()
            runs.append((model, tr, np.array(losses), stats))
    (m_e, tr_e, l_e, s_e), (m_g, tr_g, l_g, s_g) = runs
    assert tr_e.graph_replays == 0
    assert tr_g._graph is not None and tr_g.graph_replays == steps - 2 and tr_g._graph["sg"].n_segments() == 1
    np.testing.assert_allclose(l_g[:2], l_e[:2], rtol=1e-6)
    np.testing.assert_allclose(l_g, l_e, rtol=2e-3, atol=2e-4)
    for (n1, p1), (_, p2) in zip(m_g.named_parameters(), m_e.named_parameters()):
        a, b = p1.detach().float(), p2.detach().float()
        assert float((a - b).norm()) <= 2e-3 * float(b.norm()) + 0.05 * 2e-4 * steps * a.numel() ** 0.5, n1
    print("eager", [(round(s["norm"], 5), round(s["coef"], 5)) for s in s_e])
    print("graph", [(round(s["norm"], 5), round(s["coef"], 5)) for s in s_g])
    assert s_g[7]["norm"] != s_g[2]["norm"]                                  # replays refresh the statistics block
    assert all(s["coef"] < 1.0 for s in s_g[:1]) and s_g[7]["finite"]
    assert s_e[7]["skipped"] == 0 and s_g[7]["skipped"] == 0


def test_checkpoint_carries_the_skip_counter(dev):
    from dynamicvectorquantization_amd import runtime as rt
    with rt.compute_dtype_ctx(torch.float32):
        _, tr_a = _make(dev, False, gradient_clip_val=1.0, skip_nonfinite=True)
        tr_a.opts[0].flat.flat_g[3] = float("nan")
        tr_a.opts[0].step()                                                  # a real skipped step
        ckpt = tr_a.state_dict()
        assert ckpt["grad_guard"] == {"skipped": [1]}
        _, tr_plain = _make(dev, False)
        assert "grad_guard" not in tr_plain.state_dict()
        tr_plain.load_state_dict(ckpt)                                       # the extra key is tolerated
        assert tr_plain.grad_stats() == [None]
        _, tr_b = _make(dev, False, skip_nonfinite=True)
        assert tr_b.grad_stats()[0]["skipped"] == 0
        tr_b.load_state_dict(ckpt)
        assert tr_b.grad_stats()[0]["skipped"] == 1
        tr_b.load_state_dict(tr_plain.state_dict())                          # a checkpoint without the key: the counter stays
        assert tr_b.grad_stats()[0]["skipped"] == 1
