"""Weight EMA (docs/design/20-weight-ema.md): dvq_ema_update and dvq_swap_f32 against fp64 / exact exchange, HipAdam.set_weight_ema
against the fp64 recursion over the optimizer's own parameter snapshots, and the Trainer's eager / recorded / scope / checkpoint /
validation paths.  `pytest -m gpu`."""
import warnings

import numpy as np
import pytest
import torch

from dynamicvectorquantization_amd import synth

pytestmark = pytest.mark.gpu

SIZES = (1, 3, 4, 5, 1023, 1024, 1025, 65536 + 7)
OMS = (9.0 / 11.0, 1e-4)                   # 1 - d: d = 2/11 (the first warmed-up update), d = 0.9999
DECAY = 0.999


def _scaled_normal(rs, n):
    """N(0,1) times per-block scales 1e-6 .. 1e2 (blocks of ~n/7 elements)"""
    x = rs.standard_normal(n).astype(np.float32)
    edges = np.linspace(0, n, 8).astype(np.int64)
    for a, b in zip(edges[:-1], edges[1:]):
        x[a:b] *= np.float32(10.0 ** rs.randint(-6, 3))
    return x


def _dev_buf(dev, x, offset):
    """x on the device at a 16-byte aligned base (offset 0) or one element past it (offset 1: `buf[1:]`)"""
    buf = torch.zeros(x.size + 4, dtype=torch.float32, device=dev)
    assert buf.data_ptr() % 16 == 0
    view = buf[offset:offset + x.size]
    view.copy_(torch.from_numpy(x))
    assert view.data_ptr() % 16 == 4 * offset
    return buf, view


def _rec(dev, om):
    return torch.tensor([om] + [0.0] * 7, dtype=torch.float32, device=dev)


# ---- 1. kernel against fp64 ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("offset", [0, 1])
def test_ema_update_matches_fp64(dev, offset):
    """bound 2^-21 * max(|e|, |p|) per element: e - p is one fp32 rounding of a value <= 2 max, the fma one rounding of a value <= max,
    om <= 1 -- at most 3 * 2^-24 * max (5 * 2^-24 without the fma)"""
    from dynamicvectorquantization_amd import kernels as K
    rs = np.random.RandomState(21)
    for n in SIZES:
        for om in OMS:
            e0, p0 = _scaled_normal(rs, n), _scaled_normal(rs, n)
            same = rs.rand(n) < 0.25
            same[0] = n > 1 or same[0]
            p0[same] = e0[same]                                                # fixed points: p == e
            rec = _rec(dev, om)
            om32 = float(rec.cpu()[0])                                        # what the kernel reads: om rounded to fp32 once
            ebuf, e = _dev_buf(dev, e0, offset)
            pbuf, p = _dev_buf(dev, p0, offset)
            K.ema_update(e, p, rec)
            got = e.cpu().numpy()
            want = e0.astype(np.float64) - om32 * (e0.astype(np.float64) - p0.astype(np.float64))
            bound = 2.0 ** -21 * np.maximum(np.abs(e0), np.abs(p0)).astype(np.float64)
            err = np.abs(got.astype(np.float64) - want)
            worst = float((err / np.maximum(bound, 1e-300)).max())
            print(f"n={n} om={om:.4g} offset={offset}: worst err / bound {worst:.3g}")
            assert np.all(err <= bound), (n, om, offset, worst)
            assert np.array_equal(got[same].view(np.int32), e0[same].view(np.int32)), (n, om)      # fixed point, bit for bit
            assert np.array_equal(p.cpu().numpy().view(np.int32), p0.view(np.int32))                # p is read only
            guard = torch.cat([ebuf[:offset], ebuf[offset + n:]]).cpu().numpy()
            assert not guard.any(), (n, offset)                                                    # nothing written outside [0, n)
            _, e2 = _dev_buf(dev, e0, offset)                                  # determinism: the same launch from equal inputs
            K.ema_update(e2, p, rec)
            assert torch.equal(e2, e), (n, om)
            if not same.all():
                assert not np.array_equal(got, e0)


# ---- 2. the guard's skip flag -----------------------------------------------------------------------------------------------------
def test_ema_update_follows_the_skip_flag(dev):
    from dynamicvectorquantization_amd import kernels as K
    rs = np.random.RandomState(22)
    n = 1025
    e0, p0 = _scaled_normal(rs, n), _scaled_normal(rs, n)
    g = rs.standard_normal(n).astype(np.float32)
    bad = g.copy()
    bad[77] = np.nan
    ws = torch.empty(K.grad_sqnorm_workspace_bytes(n) // 8, dtype=torch.float64, device=dev)
    rec = _rec(dev, 0.25)
    for offset in (0, 1):
        _, p = _dev_buf(dev, p0, offset)
        _, e = _dev_buf(dev, e0, offset)
        gstat = K.grad_sqnorm(torch.from_numpy(bad).to(dev), ws, K.grad_stats_block(dev), 0.0, True)
        assert K.read_grad_stats(gstat)["skipped"] == 1
        K.ema_update(e, p, rec, gstat)
        assert np.array_equal(e.cpu().numpy().view(np.int32), e0.view(np.int32))                    # skipped: bit for bit
        gstat = K.grad_sqnorm(torch.from_numpy(g).to(dev), ws, gstat, 0.0, True)
        K.ema_update(e, p, rec, gstat)
        _, ref = _dev_buf(dev, e0, offset)
        K.ema_update(ref, p, rec)
        assert torch.equal(e, ref) and not np.array_equal(e.cpu().numpy(), e0)                      # finite: the update goes through
        # clipping without the guard never skips, NaN or not
        gstat = K.grad_sqnorm(torch.from_numpy(bad).to(dev), ws, K.grad_stats_block(dev), 1.0, False)
        _, e3 = _dev_buf(dev, e0, offset)
        K.ema_update(e3, p, rec, gstat)
        assert torch.equal(e3, ref)


# ---- 3. swap ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("offset", [0, 1])
def test_swap_exchanges_exactly(dev, offset):
    from dynamicvectorquantization_amd import _lib
    from dynamicvectorquantization_amd import kernels as K
    rs = np.random.RandomState(23)
    for n in SIZES:
        a0, b0 = _scaled_normal(rs, n), _scaled_normal(rs, n)
        a0[0], b0[n - 1] = np.float32(np.nan), np.float32(-0.0)               # bit patterns, not values
        abuf, a = _dev_buf(dev, a0, offset)
        bbuf, b = _dev_buf(dev, b0, offset)
        K.swap_f32(a, b)
        assert np.array_equal(a.cpu().numpy().view(np.int32), b0.view(np.int32)), n
        assert np.array_equal(b.cpu().numpy().view(np.int32), a0.view(np.int32)), n
        for buf in (abuf, bbuf):
            assert not torch.cat([buf[:offset], buf[offset + n:]]).cpu().numpy().any(), n
        K.swap_f32(a, b)                                                       # twice: the identity
        assert np.array_equal(a.cpu().numpy().view(np.int32), a0.view(np.int32)), n
        assert np.array_equal(b.cpu().numpy().view(np.int32), b0.view(np.int32)), n
    buf = torch.arange(64, dtype=torch.float32, device=dev)
    keep = buf.clone()
    for lo_a, lo_b, n in ((0, 0, 16), (0, 8, 16), (8, 0, 16), (0, 15, 16), (3, 4, 2)):
        with pytest.raises(_lib.DvqError):
            K.swap_f32(buf[lo_a:lo_a + n], buf[lo_b:lo_b + n])
    assert torch.equal(buf, keep)
    K.swap_f32(buf[0:16], buf[16:32])                                          # adjacent ranges do not overlap
    assert torch.equal(buf[0:16], keep[16:32]) and torch.equal(buf[16:32], keep[0:16])


# ---- the fp64 recursion -------------------------------------------------------------------------------------------------------------
def _recursion(p0, snaps, decay, warmup):
    """e_0 = p_0, e_n = e_{n-1} - (1 - d_n) (e_{n-1} - p_n) in fp64 over the parameter snapshots after each step"""
    from dynamicvectorquantization_amd.trainer import ema_decay_at
    e = p0.double().cpu().numpy()
    for n, p in enumerate(snaps, start=1):
        om = float(np.float32(1.0 - ema_decay_at(n, decay, warmup)))          # rounded to fp32 once, as uploaded
        e = e - om * (e - p.double().cpu().numpy())
    return e


def _assert_recursion(flat_e, p0, snaps, decay, warmup, what):
    want = _recursion(p0, snaps, decay, warmup)
    top = max(float(np.abs(want).max()), max(float(s.abs().max()) for s in [p0] + snaps))
    bound = len(snaps) * 2.0 ** -21 * top                                      # 2^-21 * max per update (test 1), N updates
    err = float(np.abs(flat_e.double().cpu().numpy() - want).max())
    print(f"{what}: max err {err:.3g}, bound {bound:.3g} ({len(snaps)} updates)")
    assert err <= bound, what


# ---- 4. HipAdam.set_weight_ema ----------------------------------------------------------------------------------------------------
def _adam_pair(dev, rs):
    from dynamicvectorquantization_amd.trainer import HipAdam
    from test_gpu_gradclip import SHAPES
    p0 = [rs.standard_normal(s).astype(np.float32) for s in SHAPES]
    out = []
    for _ in range(2):
        ps = [torch.nn.Parameter(torch.from_numpy(a.copy()).to(dev)) for a in p0]
        opt = HipAdam([{"params": ps[:3], "weight_decay": 0.01}, {"params": ps[3:], "weight_decay": 0.0}], lr=1e-2, betas=(0.9, 0.95))
        opt.flatten()
        out.append((ps, opt))
    return SHAPES, out


def test_hip_adam_weight_ema(dev):
    from dynamicvectorquantization_amd.trainer import FlatParams
    rs = np.random.RandomState(24)
    shapes, ((ema_p, ema_opt), (bare_p, bare_opt)) = _adam_pair(dev, rs)
    ema_opt.set_weight_ema(DECAY, warmup=True)
    assert ema_opt.flat_e.dtype == torch.float32 and ema_opt.flat_e.shape == ema_opt.flat.flat_p.shape
    assert torch.equal(ema_opt.flat_e, ema_opt.flat.flat_p) and ema_opt.flat_e.data_ptr() != ema_opt.flat.flat_p.data_ptr()
    assert ema_opt.ema_num_updates == 0 and bare_opt.ema_num_updates == 0 and bare_opt.ema_tensors() == {}
    p_init = ema_opt.flat.flat_p.clone()
    snaps = []
    for t in range(1, 6):
        for opt in (ema_opt, bare_opt):
            for grp in opt.param_groups:
                grp["lr"] = 1e-2 * (0.5 + 0.25 * t)
        grads = [rs.standard_normal(s).astype(np.float32) * (10.0 ** rs.randint(-3, 2)) for s in shapes]
        for a, b, g in zip(ema_p, bare_p, grads):
            a.grad.copy_(torch.from_numpy(g).to(dev))
            b.grad.copy_(torch.from_numpy(g).to(dev))
        ema_opt.step()
        bare_opt.step()
        snaps.append(ema_opt.flat.flat_p.clone())
        assert ema_opt.ema_num_updates == t
    assert not torch.equal(ema_opt.flat_e, ema_opt.flat.flat_p)
    _assert_recursion(ema_opt.flat_e, p_init, snaps, DECAY, True, "HipAdam, 5 steps")
    # the Adam kernels and their results do not change
    assert torch.equal(ema_opt.flat.flat_p, bare_opt.flat.flat_p)
    assert torch.equal(ema_opt._fstate["m"], bare_opt._fstate["m"]) and torch.equal(ema_opt._fstate["v"], bare_opt._fstate["v"])
    # views: logical shapes, the 3x3 conv weight through its channel-last storage
    views = ema_opt.ema_tensors()
    off = 0
    for p in ema_p:
        v = views[id(p)]
        assert tuple(v.shape) == tuple(p.shape)
        assert torch.equal(v, FlatParams._view(ema_opt.flat_e, off, p))
        off += p.numel()
    conv = ema_p[2]
    assert conv.dim() == 4 and views[id(conv)].permute(0, 2, 3, 1).is_contiguous()
    # without the warm-up the first update already uses `decay`
    ema_opt.set_weight_ema(0.0)
    assert ema_opt.flat_e is None and ema_opt.ema_num_updates == 0 and ema_opt.ema_tensors() == {}
    ema_opt.set_weight_ema(0.5, warmup=False)
    before = ema_opt.flat.flat_p.clone()
    ema_opt.step()
    _assert_recursion(ema_opt.flat_e, before, [ema_opt.flat.flat_p.clone()], 0.5, False, "no warm-up, 1 step")


def test_hip_adam_skipped_step_leaves_the_average(dev):
    rs = np.random.RandomState(25)
    shapes, ((ps, opt), _) = _adam_pair(dev, rs)
    opt.set_grad_guard(0.0, True)
    opt.set_weight_ema(DECAY)
    for step, poison in enumerate((False, True)):
        for p, s in zip(ps, shapes):
            p.grad.copy_(torch.from_numpy(rs.standard_normal(s).astype(np.float32)).to(dev))
        if poison:
            opt.flat.flat_g[5] = float("nan")
        before = [x.clone() for x in (opt.flat.flat_p, opt._fstate["m"], opt._fstate["v"], opt.flat_e)]
        opt.step()
        after = (opt.flat.flat_p, opt._fstate["m"], opt._fstate["v"], opt.flat_e)
        assert all(torch.equal(a, b) for a, b in zip(before, after)) == poison
        assert opt.ema_num_updates == step + 1                                 # the count advances on a skipped step, like Adam's t
    assert opt.grad_stats()["skipped"] == 1


def test_set_weight_ema_argument_checks(dev):
    from dynamicvectorquantization_amd.trainer import HipAdam
    opt = HipAdam([torch.nn.Parameter(torch.zeros(5, device=dev))])
    with pytest.raises(ValueError, match="flatten"):
        opt.set_weight_ema(0.999)
    opt.flatten()
    for bad in (1.0, 1.5, -0.1, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            opt.set_weight_ema(bad)
    assert opt.flat_e is None
    opt.set_weight_ema(0.999)
    assert opt.flat_e is not None


# ---- Trainer ------------------------------------------------------------------------------------------------------------------------
def _model(dev, seed=0):
    from dynamicvectorquantization_amd.config import instantiate_from_config
    from test_gpu_model import GEOM, model_config
    torch.manual_seed(seed)
    model = instantiate_from_config(model_config(**GEOM["small"], loss="ae")).to(dev)
    model.learning_rate, model.min_learning_rate = 2e-4, 1e-5
    model.training_steps, model.steps_per_epoch, model.warmup_epochs = 12, 4, 1
    return model


def _make(dev, use_graph, graph_after=2, seed=0, **kw):
    """tests/test_gpu_gradclip.py::_make with the EMA arguments"""
    from dynamicvectorquantization_amd.trainer import Trainer
    model = _model(dev, seed).train()
    return model, Trainer(model, max_steps=12, use_graph=use_graph, graph_after=graph_after, **kw)


def _images(dev):
    return [torch.from_numpy(synth.half_flat_images(2, 64, seed=40 + i)).to(dev) for i in range(3)]


def _run(tr, xs, steps):
    """`steps` train steps -> (p_0, [flat_p after each step])"""
    opt = tr.opts[0]
    p0, snaps = opt.flat.flat_p.clone(), []
    for i in range(steps):
        tr.train_step({"image": xs[i % 3]}, i)
        snaps.append(opt.flat.flat_p.clone())
    torch.cuda.synchronize()
    assert not torch.equal(opt.flat_e, opt.flat.flat_p)                        # no comparison below is vacuous
    return p0, snaps


def _fresh_with(dev, state_dict):
    model = _model(dev, seed=123)                                              # other initial weights: everything comes from the file
    model.load_state_dict(state_dict)
    return model.eval()


# ---- 5. the recorded step follows the schedule ------------------------------------------------------------------------------------
def test_recorded_step_follows_the_decay_schedule(dev):
    """d_n differs at every one of the 8 steps (2/11, 3/12, ...): a replay that baked the decay of the first replayed step into its
    launch misses the recursion"""
    from dynamicvectorquantization_amd import runtime as rt
    from dynamicvectorquantization_amd.trainer import ema_decay_at
    assert len({ema_decay_at(n, DECAY, True) for n in range(1, 9)}) == 8
    xs, steps = _images(dev), 8
    with rt.compute_dtype_ctx(torch.float32):
        for use_graph in (True, False):
            model, tr = _make(dev, use_graph, ema_decay=DECAY)
            assert len(tr.opts) == 1
            p0, snaps = _run(tr, xs, steps)
            _assert_recursion(tr.opts[0].flat_e, p0, snaps, DECAY, True, f"trainer, use_graph={use_graph}")
            assert tr.opts[0].ema_num_updates == steps
            if use_graph:
                assert tr._graph is not None and tr.graph_replays == steps - 2 and tr._graph["sg"].n_segments() == 1
            else:
                assert tr.graph_replays == 0


# ---- 6. ema_scope -----------------------------------------------------------------------------------------------------------------
def _encode(model, x):
    with torch.no_grad():
        codes = model.encode(x)[2][-1].clone()
        rec = model(x)[0].clone()
    return codes, rec


def test_ema_scope(dev):
    from dynamicvectorquantization_amd import evaluate as E
    from dynamicvectorquantization_amd import runtime as rt
    xs = _images(dev)
    with rt.compute_dtype_ctx(torch.float32):
        model, tr = _make(dev, False, ema_decay=DECAY)
        _run(tr, xs, 4)
        opt = tr.opts[0]
        ckpt = tr.state_dict()
        ref = _fresh_with(dev, E.checkpoint_state_dict(ckpt, use_ema=True))
        want_codes, want_rec = _encode(ref, xs[0])
        live_p, live_e = opt.flat.flat_p.clone(), opt.flat_e.clone()
        ptr = opt.flat.flat_p.data_ptr()
        model.eval()
        before_codes, before_rec = _encode(model, xs[0])                       # packs the LIVE weights: stale inside the scope
        with tr.ema_scope():
            assert torch.equal(opt.flat.flat_p, live_e) and torch.equal(opt.flat_e, live_p)
            assert opt.flat.flat_p.data_ptr() == ptr                            # no pointer moves
            codes, rec = _encode(model, xs[0])
            assert torch.equal(codes, want_codes) and torch.equal(rec, want_rec)
            with pytest.raises(RuntimeError, match="ema_scope"):
                tr.train_step({"image": xs[1]}, 4)
            with pytest.raises(RuntimeError, match="nest"):
                with tr.ema_scope():
                    pass
        assert torch.equal(opt.flat.flat_p, live_p) and torch.equal(opt.flat_e, live_e)
        after_codes, after_rec = _encode(model, xs[0])
        assert torch.equal(after_codes, before_codes) and torch.equal(after_rec, before_rec)
        assert not torch.equal(rec, before_rec)                                # the two sets of weights do differ in what they compute
        with pytest.raises(KeyError):                                          # the body raises: the weights still come back
            with tr.ema_scope():
                raise KeyError("body")
        assert torch.equal(opt.flat.flat_p, live_p) and torch.equal(opt.flat_e, live_e)
        model.train()
        tr.train_step({"image": xs[1]}, 4)                                     # and training goes on
        # feature off: a no-op
        plain_model, plain = _make(dev, False)
        keep = plain.opts[0].flat.flat_p.clone()
        with plain.ema_scope():
            assert torch.equal(plain.opts[0].flat.flat_p, keep) and plain.opts[0].flat_e is None
            plain.train_step({"image": xs[0]}, 0)                              # nothing to protect


# ---- 7. checkpoint ------------------------------------------------------------------------------------------------------------------
def test_checkpoint_round_trip(dev):
    from dynamicvectorquantization_amd import runtime as rt
    xs = _images(dev)
    with rt.compute_dtype_ctx(torch.float32):
        model_a, tr_a = _make(dev, False, ema_decay=DECAY)
        _run(tr_a, xs, 3)
        ckpt = tr_a.state_dict()
        ema = ckpt["ema"]
        assert ema["decay"] == DECAY and ema["warmup"] is True and ema["num_updates"] == 3
        names = dict(model_a.named_parameters())
        by_id = {id(p): k for k, p in names.items()}
        assert set(ema["state_dict"]) == {by_id[id(p)] for p in tr_a.opts[0].flat.params}      # exactly optimizer 0's parameters
        assert set(ema["state_dict"]) <= set(ckpt["state_dict"])
        w, b = ema["state_dict"]["decoder.conv_out.weight"], ema["state_dict"]["decoder.conv_out.bias"]
        assert tuple(w.shape) == tuple(names["decoder.conv_out.weight"].shape) and w.shape[2:] == (3, 3) and w.is_contiguous()
        assert tuple(b.shape) == tuple(names["decoder.conv_out.bias"].shape) and b.dim() == 1
        assert all(not t.is_cuda and t.is_contiguous() for t in ema["state_dict"].values())
        assert torch.equal(w.to(dev), tr_a.opts[0].ema_tensors()[id(names["decoder.conv_out.weight"])])
        assert not torch.equal(w, ckpt["state_dict"]["decoder.conv_out.weight"].cpu())

        _, tr_plain = _make(dev, False, seed=1)
        tr_plain.load_state_dict(ckpt)                                         # the extra key is ignored
        plain_ckpt = tr_plain.state_dict()
        assert "ema" not in plain_ckpt and tr_plain.opts[0].flat_e is None

        _, tr_b = _make(dev, False, seed=2, ema_decay=0.99)                     # the decay of THIS run applies
        tr_b.load_state_dict(ckpt)
        assert torch.equal(tr_b.opts[0].flat_e, tr_a.opts[0].flat_e) and tr_b.opts[0].ema_num_updates == 3
        assert torch.equal(tr_b.opts[0].flat.flat_p, tr_a.opts[0].flat.flat_p)
        assert tr_b.state_dict()["ema"]["decay"] == 0.99

        with pytest.warns(UserWarning, match="ema"):
            tr_b.load_state_dict(plain_ckpt)                                   # written without the feature
        assert torch.equal(tr_b.opts[0].flat_e, tr_b.opts[0].flat.flat_p) and tr_b.opts[0].ema_num_updates == 0
        assert torch.equal(tr_b.opts[0].flat.flat_p, tr_a.opts[0].flat.flat_p)
        with warnings.catch_warnings():
            warnings.filterwarnings("error", message=".*ema.*")                # warned once
            tr_b.load_state_dict(plain_ckpt)


# ---- 8. validation sees the average ---------------------------------------------------------------------------------------------------
def test_validation_uses_the_averaged_weights(dev):
    from dynamicvectorquantization_amd import evaluate as E
    from dynamicvectorquantization_amd import runtime as rt
    from dynamicvectorquantization_amd.trainer import Trainer
    xs = _images(dev)
    vs = [{"image": torch.from_numpy(synth.half_flat_images(2, 64, seed=90 + i)).to(dev)} for i in range(2)]
    with rt.compute_dtype_ctx(torch.float32):
        model, tr = _make(dev, False, ema_decay=DECAY)
        _run(tr, xs, 4)
        ckpt = tr.state_dict()
        live_p = tr.opts[0].flat.flat_p.clone()
        got = tr.validate(vs)
        assert torch.equal(tr.opts[0].flat.flat_p, live_p) and model.training and not tr._in_ema_scope

        def fresh_metrics(sd):
            m = _fresh_with(dev, sd)
            m.learning_rate, m.global_step = model.learning_rate, model.global_step
            return Trainer(m, max_steps=12, use_graph=False).validate(vs)

        want = fresh_metrics(E.checkpoint_state_dict(ckpt, use_ema=True))
        live = fresh_metrics(E.checkpoint_state_dict(ckpt))
    print("ema ", got)
    print("want", want)
    print("live", live)
    assert set(got) == set(want) and "val_rec_loss" in got                      # metric names unchanged
    for k in want:
        np.testing.assert_allclose(got[k], want[k], rtol=1e-6, err_msg=k)
    assert got["val_rec_loss"] != live["val_rec_loss"]
