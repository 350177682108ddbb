"""Per-parameter norm tracking (docs/design/24-norm-tracking.md) on the GPU: dvq_segment_stats and dvq_copy_f32_armed against the
numpy fp64 restatement (tests/normtrack_math.py), HipAdam.set_norm_tracking against norms of host copies, and the Trainer's eager /
recorded paths with the feature on and off.  `pytest -m gpu`."""
import os

import numpy as np
import pytest
import torch

from conftest import REPO, load_golden
from dynamicvectorquantization_amd import synth

import normtrack_math as NM

pytestmark = pytest.mark.gpu

SHAPES = [(37, 5), (1,), (8, 4, 3, 3), (11,), (6, 6), (130, 7)]      # of test_hip_adam_matches_torch_optim, restated
REL = 2.0 ** -53 * 4                                                  # times the segment length: the bound of tests/test_gpu_gradclip.py


def _chunk():
    from dynamicvectorquantization_amd import kernels as K
    c = K.GRAD_SQNORM_CHUNK
    assert K.grad_sqnorm_workspace_bytes(c) == 8 and K.grad_sqnorm_workspace_bytes(c + 1) == 16      # the library's own chunk length
    return c


def _lengths():
    c = _chunk()
    return [1, 3, 4, 5, c - 1, c, c + 1, 2 * c + 7, 2, 1]


def _values(rs, n):
    """N(0,1) times per-block scales 1e-6 .. 1e2, plus a few +-1e25 entries whose fp32 squares overflow"""
    x = rs.standard_normal(n).astype(np.float32)
    edges = np.linspace(0, n, 10).astype(np.int64)
    for i, (a, b) in enumerate(zip(edges[:-1], edges[1:])):
        x[a:b] *= np.float32(10.0 ** (i - 6))
    big = rs.choice(n, 6, replace=False)
    x[big] = np.float32(1e25) * np.where(np.arange(6) % 2 == 0, 1, -1).astype(np.float32)
    return x


class _Case:
    """one buffer of the ten segment lengths on the device, aligned (off = 0) or as a view starting one element in (off = 1)"""

    def __init__(self, dev, off):
        from dynamicvectorquantization_amd import kernels as K
        self.K, self.dev, self.off = K, dev, off
        self.lengths = _lengths()
        self.offsets = NM.offsets_of(self.lengths)
        self.n, self.S = int(self.offsets[-1]), len(self.lengths)
        self.plan = K.SegmentPlan(self.offsets, dev)
        self.ws = K.segment_stats_workspace(self.n, self.S, dev)
        assert self.plan.nchunks == sum(-(-l // _chunk()) for l in self.lengths) == 13

    def dev_buf(self, x):
        base = torch.zeros(self.n + 4, dtype=torch.float32, device=self.dev)
        view = base[self.off:self.off + self.n]
        view.copy_(torch.from_numpy(x))
        assert view.data_ptr() % 16 == 4 * self.off
        return view

    def run(self, x, y=None, state=None, sticky=False, armed=None):
        K = self.K
        state = K.segment_stats_state(self.S, self.dev) if state is None else state
        K.segment_stats(self.dev_buf(x), None if y is None else self.dev_buf(y), self.plan, self.ws, state, sticky=sticky, armed=armed)
        return state

    def read(self, state):
        return {k: v.numpy().copy() for k, v in self.K.segment_stats_views(state.cpu(), self.S).items()}


def _check(case, got, x, y=None, tag=""):
    sumsq, absmax, bad = NM.segment_stats(x, case.offsets, y)
    for s, ln in enumerate(case.lengths):
        err = abs(got["sumsq"][s] - sumsq[s]) / sumsq[s] if sumsq[s] > 0 else abs(got["sumsq"][s])
        print(f"{tag} segment {s} len {ln}: sumsq {got['sumsq'][s]:.17g} fp64 {sumsq[s]:.17g} rel err {err:.3g} bound {ln * REL:.3g}")
        assert err <= ln * REL, (tag, s)
    assert np.array_equal(got["absmax"], absmax), tag
    assert np.array_equal(got["nonfinite"], bad), tag


@pytest.mark.parametrize("off", [0, 1], ids=["aligned", "misaligned"])
def test_segment_stats_match_fp64(dev, off):
    """ten segments around the chunk length and the 16-byte vector; only the ORDER of the fp64 additions differs from numpy's.  Plain
    and difference mode; the same input twice gives bit-equal state blocks; aligned and misaligned base give the same bits"""
    case = _Case(dev, off)
    rs = np.random.RandomState(31)
    x, y = _values(rs, case.n), _values(rs, case.n)
    with np.errstate(over="ignore"):
        assert not np.isfinite(np.float32(1e25) * np.float32(1e25))
    st = case.run(x)
    got = case.read(st)
    _check(case, got, x, tag=f"plain off={off}")
    assert np.array_equal(got["nonfinite"], np.zeros(case.S, np.int64))
    assert torch.equal(st, case.run(x))
    sd = case.run(x, y)
    _check(case, case.read(sd), x, y, tag=f"diff off={off}")
    assert torch.equal(sd, case.run(x, y))
    other = _Case(dev, 1 - off)                      # the element-to-accumulator assignment is a function of the chunk alone
    assert torch.equal(st, other.run(x)) and torch.equal(sd, other.run(x, y))
    # non-sticky launches leave the sticky fields as the caller set them
    assert np.array_equal(got["nonfinite_total"], np.zeros(case.S, np.int64)) and np.array_equal(got["first_bad_call"], -np.ones(case.S, np.int64))
    assert np.array_equal(got["calls"], np.zeros(case.S, np.int64))


@pytest.mark.parametrize("off", [0, 1], ids=["aligned", "misaligned"])
def test_nonfinite_elements_are_counted_and_left_out(dev, off):
    """Inf / NaN at first, last, chunk-boundary and tail positions of chosen segments: exact counts, the other segments bit for bit as
    in the clean run, the sticky counters over three launches (clean, bad, clean)"""
    c = _chunk()
    case = _Case(dev, off)
    o = case.offsets
    rs = np.random.RandomState(32)
    x = _values(rs, case.n)
    bad = x.copy()
    plant = {1: [0, 2], 4: [c - 2], 6: [c - 1, c], 7: [0, c, 2 * c - 1, 2 * c, 2 * c + 4, 2 * c + 6], 9: [0]}      # segment -> positions in it
    vals = [np.nan, np.inf, -np.inf]
    k = 0
    for s, pos in plant.items():
        for p in pos:
            assert p < case.lengths[s]
            bad[o[s] + p] = vals[k % 3]
            k += 1
    state = case.K.segment_stats_state(case.S, dev)
    clean = case.read(case.run(x, state=state, sticky=True))
    got = case.read(case.run(bad, state=state, sticky=True))
    _check(case, got, bad, tag=f"planted off={off}")
    want = np.array([len(plant.get(s, [])) for s in range(case.S)], np.int64)
    assert np.array_equal(got["nonfinite"], want)
    for s in range(case.S):
        if s not in plant:
            assert got["sumsq"][s].tobytes() == clean["sumsq"][s].tobytes() and got["absmax"][s].tobytes() == clean["absmax"][s].tobytes(), s
    after = case.read(case.run(x, state=state, sticky=True))
    total, first = NM.sticky([np.zeros(case.S, np.int64), want, np.zeros(case.S, np.int64)])
    assert np.array_equal(after["nonfinite_total"], total) and np.array_equal(after["first_bad_call"], first)
    assert np.array_equal(after["calls"], np.full(case.S, 3, np.int64)) and np.array_equal(after["nonfinite"], np.zeros(case.S, np.int64))
    assert after["sumsq"].tobytes() == clean["sumsq"].tobytes() and after["absmax"].tobytes() == clean["absmax"].tobytes()
    # difference mode: a non-finite element in either operand counts, once
    d = case.read(case.run(x, bad))
    assert np.array_equal(d["nonfinite"], want)
    _check(case, d, x, bad, tag=f"diff planted off={off}")


def test_unarmed_launches_touch_nothing(dev):
    from dynamicvectorquantization_amd import kernels as K
    case = _Case(dev, 0)
    rs = np.random.RandomState(33)
    x = _values(rs, case.n)
    armed = torch.zeros(1, dtype=torch.int32, device=dev)
    sentinel = torch.full((K.segment_stats_state(case.S, dev).numel(),), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device=dev)
    state = sentinel.clone()
    case.ws.fill_(0x1234)
    case.run(x, state=state, sticky=True, armed=armed)
    assert torch.equal(state, sentinel) and bool((case.ws == 0x1234).all())
    src, dst = case.dev_buf(x), torch.full((case.n,), 7.0, device=dev)
    K.copy_f32_armed(dst, src, armed)
    assert bool((dst == 7.0).all())
    armed.fill_(1)
    K.copy_f32_armed(dst, src, armed)
    assert dst.cpu().numpy().tobytes() == x.tobytes()
    for off in (1, 2):                                               # the 4-byte path, odd lengths
        d2 = torch.full((case.n,), 7.0, device=dev)
        K.copy_f32_armed(d2[off:off + 1001], src[3:1004], None)
        h = d2.cpu().numpy()
        assert h[off:off + 1001].tobytes() == x[3:1004].tobytes() and (h[:off] == 7.0).all() and (h[off + 1001:] == 7.0).all()
    got = case.read(case.run(x, state=K.segment_stats_state(case.S, dev), armed=armed))
    _check(case, got, x, tag="armed")


def test_bad_tables_are_refused_before_any_launch(dev):
    import ctypes as C
    from dynamicvectorquantization_amd import kernels as K
    from dynamicvectorquantization_amd._lib import DvqError
    case = _Case(dev, 0)
    lib = K.lib()
    x = case.dev_buf(np.ones(case.n, np.float32))
    sentinel = torch.full((K.segment_stats_state(case.S, dev).numel(),), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device=dev)
    state = sentinel.clone()

    def call(offsets, S, n, ws_bytes=None, plan_bytes=None):
        arr = (C.c_int64 * len(offsets))(*[int(v) for v in offsets])
        return lib.dvq_segment_stats(x.data_ptr(), None, n, arr, S, case.plan.plan.data_ptr(),
                                     case.plan.plan_bytes if plan_bytes is None else plan_bytes, case.ws.data_ptr(),
                                     case.ws.numel() * 8 if ws_bytes is None else ws_bytes, state.data_ptr(), 1, None, None)

    good = list(case.offsets)
    swapped = good[:]
    swapped[3], swapped[4] = swapped[4], swapped[3]
    empty = good[:]
    empty[5] = empty[4]
    assert call(swapped, case.S, case.n) == -2                       # DVQ_ESHAPE: not ascending
    assert call(empty, case.S, case.n) == -2                         # a segment of length 0
    assert call(good[:-1] + [case.n - 1], case.S, case.n) == -2      # does not end at n
    assert call([1] + good[1:], case.S, case.n) == -2                # does not start at 0
    assert call(good, case.S, case.n, plan_bytes=case.plan.plan_bytes - 16) == -2      # a plan of another table
    assert call(good, case.S, case.n, ws_bytes=16 * case.plan.nchunks - 8) == -5       # DVQ_EWORKSPACE
    torch.cuda.synchronize()
    assert torch.equal(state, sentinel)                              # nothing was launched
    assert call(good, case.S, case.n, ws_bytes=16 * case.plan.nchunks) == 0
    torch.cuda.synchronize()
    assert not torch.equal(state, sentinel)
    with pytest.raises(DvqError):
        K.SegmentPlan(swapped, dev)
    assert lib.dvq_segment_stats_workspace_bytes(case.n, case.S) >= 16 * case.plan.nchunks


def test_many_one_element_segments(dev):
    """S = 65535 segments of one element each: every row is that element's square"""
    from dynamicvectorquantization_amd import kernels as K
    S = 65535
    plan = K.SegmentPlan(range(S + 1), dev)
    rs = np.random.RandomState(34)
    x = rs.standard_normal(S).astype(np.float32)
    state = K.segment_stats_state(S, dev)
    K.segment_stats(torch.from_numpy(x).to(dev), None, plan, K.segment_stats_workspace(S, S, dev), state)
    got = K.segment_stats_views(state.cpu(), S)
    assert np.array_equal(got["sumsq"].numpy(), x.astype(np.float64) ** 2) and np.array_equal(got["absmax"].numpy(), np.abs(x))


# ---- HipAdam ---------------------------------------------------------------------------------------------------------------------
def _optimizer(dev, rs, guard=None, track_updates=True):
    from dynamicvectorquantization_amd.trainer import HipAdam
    p0 = [rs.standard_normal(s).astype(np.float32) * (1e-3 if i == 3 else 1.0) for i, s in enumerate(SHAPES)]
    ps = [torch.nn.Parameter(torch.from_numpy(a.copy()).to(dev)) for a in p0]
    opt = HipAdam([{"params": ps[:3], "weight_decay": 0.01}, {"params": ps[3:], "weight_decay": 0.0}], lr=1e-3, betas=(0.9, 0.95))
    opt.flatten()
    if guard is not None:
        opt.set_grad_guard(*guard)
    names = {id(p): f"layer{i // 2}.p{i}" for i, p in enumerate(ps)}
    opt.set_norm_tracking(names, track_updates)
    return ps, opt, [names[id(p)] for p in ps]


def _norm64(a):
    return float(np.sqrt(np.sum(np.asarray(a, np.float32).astype(np.float64) ** 2)))


def _close(got, want, numel):
    return abs(got - want) <= want * numel * REL if want > 0 else got == 0.0


def test_optimizer_norms_match_host_copies(dev):
    """gradients filled on the host, one armed step: per-parameter grad / weight / update norms equal numpy norms of the host copies
    (p.grad, p after, p after - p before) -- the 4-D conv weight, stored channel-last, through its logical tensor.  (The norm is the
    square root of a sum within len * 2^-53 * 4: half that relative error, so the bound on the sum holds for the norm.)"""
    rs = np.random.RandomState(41)
    ps, opt, names = _optimizer(dev, rs)
    assert ps[2].dim() == 4 and not ps[2].data.is_contiguous()
    for t in range(2):
        grads = [rs.standard_normal(s).astype(np.float32) * (10.0 ** rs.randint(-6, 2)) for s in SHAPES]
        grads[4][:] = 0.0
        for p, g in zip(ps, grads):
            p.grad.copy_(torch.from_numpy(g).to(dev))
        before = [p.detach().cpu().numpy().copy() for p in ps]
        opt.arm_norm_row(True)
        opt.step()
        stats = opt.norm_stats()
        assert list(stats) == names
        for p, g, b, n in zip(ps, grads, before, names):
            e, after = stats[n], p.detach().cpu().numpy()
            assert e["numel"] == p.numel() and e["grad_nonfinite"] == 0 and e["grad_nonfinite_total"] == 0 and e["first_bad_step"] == -1
            upd = after.astype(np.float64) - b.astype(np.float64)
            print(f"t={t} {n}: grad {e['grad_norm']:.17g} / {_norm64(g):.17g} weight {e['weight_norm']:.17g} / {_norm64(after):.17g} "
                  f"update {e['update_norm']:.17g} / {float(np.sqrt(np.sum(upd * upd))):.17g}")
            assert _close(e["grad_norm"], _norm64(g), p.numel()), n
            assert e["grad_absmax"] == float(np.abs(g).max()), n
            assert _close(e["weight_norm"], _norm64(after), p.numel()), n
            assert _close(e["update_norm"], float(np.sqrt(np.sum(upd * upd))), p.numel()), n
            assert e["update_ratio"] == e["update_norm"] / e["weight_norm"]
    # an unarmed step: gradient entries move, weight / update entries stay
    for p in ps:
        p.grad.copy_(torch.from_numpy(rs.standard_normal(tuple(p.shape)).astype(np.float32)).to(dev))
    opt.arm_norm_row(False)
    opt.step()
    later = opt.norm_stats()
    for n in names:
        assert later[n]["weight_norm"] == stats[n]["weight_norm"] and later[n]["update_norm"] == stats[n]["update_norm"]
        assert later[n]["grad_norm"] != stats[n]["grad_norm"]


def test_optimizer_names_the_parameter_with_the_nan(dev):
    """guard on, a NaN and an Inf planted in one parameter's gradient at step 2 (0-based): the step is skipped, every update norm is
    0, and norm_stats() names exactly that parameter with the right count and step"""
    rs = np.random.RandomState(42)
    ps, opt, names = _optimizer(dev, rs, guard=(0.0, True))
    for t in range(4):
        grads = [rs.standard_normal(s).astype(np.float32) for s in SHAPES]
        if t == 2:
            grads[5][17, 3] = np.nan
            grads[5][129, 6] = np.inf
        for p, g in zip(ps, grads):
            p.grad.copy_(torch.from_numpy(g).to(dev))
        before = opt.flat.flat_p.clone()
        opt.arm_norm_row(True)
        opt.step()
        stats = opt.norm_stats()
        if t == 2:
            assert torch.equal(before, opt.flat.flat_p) and opt.grad_stats()["skipped"] == 1
            assert all(stats[n]["update_norm"] == 0.0 and stats[n]["update_ratio"] == 0.0 for n in names)
            assert [n for n in names if stats[n]["grad_nonfinite"]] == [names[5]] and stats[names[5]]["grad_nonfinite"] == 2
            finite = grads[5].astype(np.float64)[np.isfinite(grads[5])]
            assert _close(stats[names[5]]["grad_norm"], float(np.sqrt(np.sum(finite * finite))), ps[5].numel())
        else:
            assert all(stats[n]["update_norm"] > 0.0 for n in names) and all(stats[n]["grad_nonfinite"] == 0 for n in names)
    assert [n for n in names if stats[n]["grad_nonfinite_total"]] == [names[5]]
    assert stats[names[5]]["grad_nonfinite_total"] == 2 and stats[names[5]]["first_bad_step"] == 2
    assert all(stats[n]["first_bad_step"] == -1 for n in names[:5])
    from dynamicvectorquantization_amd import normtrack
    line, total = normtrack.nonfinite_report(0, stats, 0)
    assert total == 2 and names[5] in line and "2 elements" in line and "step 2" in line


def test_norm_tracking_needs_a_flattened_optimizer(dev):
    from dynamicvectorquantization_amd.trainer import HipAdam
    ps = [torch.nn.Parameter(torch.zeros(5, device=dev))]
    opt = HipAdam(ps)
    with pytest.raises(ValueError, match="flatten"):
        opt.set_norm_tracking({id(ps[0]): "w"})
    assert opt.norm_stats() is None
    opt.flatten()
    opt.set_norm_tracking({id(ps[0]): "w"}, track_updates=False)
    opt.step()
    st = opt.norm_stats()["w"]
    assert st["update_norm"] is None and st["update_ratio"] is None and st["weight_norm"] == 0.0
    opt.set_norm_tracking(None)
    assert opt.norm_stats() is None


# ---- Trainer ---------------------------------------------------------------------------------------------------------------------
STEPS, EVERY = 6, 3                    # rows behind steps 2 and 5; graph_after = 2: steps 0, 1 eager, steps 2 .. 5 replayed


def _stage1_run(dev, use_graph, steps=STEPS, **kw):
    """the `small` stage-1 model of the pinned run (two optimizers) under Trainer(deterministic=True), fp32"""
    from dynamicvectorquantization_amd import kernels as K
    from dynamicvectorquantization_amd import runtime as rt
    from dynamicvectorquantization_amd.config import instantiate_from_config
    from dynamicvectorquantization_amd.trainer import Trainer
    from golden_cfg import TRAIN_STEP
    from test_gpu_model import GEOM, model_config
    c = TRAIN_STEP["small"]
    g = GEOM[c["geom"]]
    out = {"losses": [], "stats": []}
    try:
        with rt.compute_dtype_ctx("fp32"):
            torch.manual_seed(0)
            model = instantiate_from_config(model_config(**g, loss="full", ndf=c["ndf"])).to(dev)
            synth.apply_train_step_state(model, g["k"], g["zc"])
            rt.bump_weights_epoch()
            model.learning_rate, model.min_learning_rate = c["lr"], c["min_lr"]
            model.warmup_epochs, model.steps_per_epoch, model.training_steps = c["warmup_epochs"], c["steps_per_epoch"], c["training_steps"]
            model.train()
            tr = Trainer(model, max_steps=steps, use_graph=use_graph, graph_after=2, deterministic=True, **kw)
            assert len(tr.opts) == 2
            torch.cuda.synchronize()
            c0 = K.unordered_launches()
            for step, xb in enumerate(synth.train_step_batches(steps, c["bs"], g["resolution"])):
                losses = tr.train_step({"image": torch.from_numpy(xb).to(dev)}, step)
                torch.cuda.synchronize()
                out["losses"].append([float(l) for l in losses])
                out["stats"].append(tr.norm_stats())
            out["unordered"] = K.unordered_launches() - c0
            out["params"] = [o.flat.flat_p.clone() for o in tr.opts]
            out["moments"] = [(o._fstate["m"].clone(), o._fstate["v"].clone()) for o in tr.opts]
            out["replays"] = tr.graph_replays
            out["launches"] = tr._graph["sg"].launch_counts() if tr._graph is not None else None
            out["names"] = [[n for n, p in model.named_parameters() if any(p is q for q in o.flat.params)] for o in tr.opts]
    finally:
        K.set_deterministic(False)
    return out


@pytest.fixture(scope="module")
def runs(dev, tmp_path_factory):
    d = tmp_path_factory.mktemp("norms")
    on = _stage1_run(dev, True, track_grad_norm=2, norm_every=EVERY, norm_logdir=str(d / "on"))
    off = _stage1_run(dev, True, track_grad_norm=-1, norm_every=EVERY, norm_logdir=str(d / "off"))
    eager = _stage1_run(dev, False, track_grad_norm="inf", norm_every=EVERY)
    bare = _stage1_run(dev, True, steps=3)
    return {"on": on, "off": off, "eager": eager, "bare": bare, "dir": d}


def test_trainer_tracking_is_read_only(runs):
    """(a) same seed, tracking on and off, the step recorded and replayed four times: parameters, Adam moments and losses bit-equal,
    no unordered launch in either"""
    on, off = runs["on"], runs["off"]
    assert on["replays"] == off["replays"] == STEPS - 2 >= 3
    assert on["losses"] == off["losses"]
    for a, b in zip(on["params"], off["params"]):
        assert torch.equal(a, b)
    for (m1, v1), (m2, v2) in zip(on["moments"], off["moments"]):
        assert torch.equal(m1, m2) and torch.equal(v1, v2)
    assert on["unordered"] == off["unordered"] == 0


def test_trainer_replayed_rows_equal_eager_rows(runs):
    """(b) the statistics of replayed armed steps (2 and 5) equal, bit for bit, those of an identically seeded all-eager run; every
    parameter of the model has a finite row"""
    on, eager = runs["on"], runs["eager"]
    assert eager["replays"] == 0
    for step in (EVERY - 1, 2 * EVERY - 1):
        assert on["stats"][step] == eager["stats"][step], step
    for oi, names in enumerate(on["names"]):
        st = on["stats"][STEPS - 1][oi]
        assert sorted(st) == sorted(names) and len(names) > 4
        for n, e in st.items():
            assert all(np.isfinite(e[k]) for k in ("grad_norm", "grad_absmax", "weight_norm", "update_norm", "update_ratio")), n
            assert e["weight_norm"] >= 0 and e["grad_nonfinite_total"] == 0 and e["first_bad_step"] == -1
        assert any(e["update_norm"] > 0 for e in st.values()) and any(e["grad_norm"] > 0 for e in st.values())


def test_trainer_unarmed_replays_keep_the_row(runs):
    """(c) behind the unarmed replayed steps 3 and 4 the weight and update entries are those of step 2, the gradient entries move"""
    st = runs["on"]["stats"]
    for oi in range(2):
        row, moved = st[2][oi], 0
        for step in (3, 4):
            for n, e in st[step][oi].items():
                assert e["weight_norm"] == row[n]["weight_norm"] and e["update_norm"] == row[n]["update_norm"], (step, n)
                moved += e["grad_norm"] != row[n]["grad_norm"]
        assert moved > 0
        assert any(st[5][oi][n]["weight_norm"] != row[n]["weight_norm"] for n in row)          # the next row step refreshes them


def test_trainer_off_costs_nothing(runs):
    """(d) tracking off: norm_stats() is None, the recorded step has the launch count of a Trainer built without the argument, no
    norms.csv; on: the count grows by the seven launches per optimizer, norms.csv has one line per parameter and row"""
    on, off, bare = runs["on"], runs["off"], runs["bare"]
    assert all(s is None for s in off["stats"]) and all(s is None for s in bare["stats"])
    assert off["launches"] is not None and off["launches"] == bare["launches"]
    assert on["launches"][0] == off["launches"][0] + 2 * 7 and on["launches"][1:] == off["launches"][1:]
    assert not os.path.exists(runs["dir"] / "off" / "norms.csv") and not os.path.exists(runs["dir"] / "off")
    import csv
    with open(runs["dir"] / "on" / "norms.csv", newline="") as f:
        rows = list(csv.DictReader(f))
    assert len(rows) == 2 * sum(len(n) for n in on["names"]) and {r["step"] for r in rows} == {"2", "5"}
    r = next(r for r in rows if r["step"] == "5" and r["opt"] == "1")
    assert float(r["grad_norm"]) == on["stats"][5][1][r["name"]]["grad_norm"] and r["grad_norm"] == repr(float(r["grad_norm"]))


def test_stage2_step_with_tracking(dev, tmp_path):
    """two eager steps of the small Dualformer with tracking and a metrics logger: a finite row for every trained parameter, the totals
    in the metrics row, norms.csv at depth 2 next to metrics.csv, norms/<stat>/<group> scalars in the event file"""
    from dynamicvectorquantization_amd import runtime as rt
    from dynamicvectorquantization_amd.metrics import MetricsLogger
    from dynamicvectorquantization_amd.config import instantiate_from_config
    from dynamicvectorquantization_amd.trainer import Trainer
    from golden_cfg import TRAIN_STEP_S2, dualformer_cfg, train_step_s2_batch
    from test_oracle_golden import dqvae_state_dict
    c = TRAIN_STEP_S2
    thr_json = os.path.join(REPO, "scripts/tools/thresholds/entropy_thresholds_imagenet_train_patch-16.json")
    with rt.compute_dtype_ctx("bf16"):
        torch.manual_seed(0)
        cfg = dualformer_cfg("uncond", thr_json)
        cfg["weight_decay"], cfg["warmup_epochs"] = c["weight_decay"], c["warmup_epochs"]
        model = instantiate_from_config({"target": "models.stage2_dynamic.dqtransformer_uncond_entropy.Dualformer", "params": cfg}).to(dev)
        model.first_stage_model.load_state_dict(dqvae_state_dict(load_golden("dqvae_small"), "spread", 512, 64))
        with torch.no_grad():
            for n, p in model.transformer.named_parameters():
                v = synth.det_param("dualformer.uncond." + n, tuple(p.shape))
                p.copy_(torch.from_numpy(v * (0.3 if n == "pos_emb" else 1.0)).to(dev))
        rt.bump_weights_epoch()
        model.learning_rate, model.min_learning_rate = c["lr"], c["min_lr"]
        model.steps_per_epoch, model.training_steps = c["steps_per_epoch"], c["training_steps"]
        model.train()
        lg = MetricsLogger(str(tmp_path), writers=("csv", "tensorboard"), log_every_n_steps=1)
        tr = Trainer(model, max_steps=2, use_graph=False, track_grad_norm=2, norm_every=7, norm_depth=2, metrics_logger=lg)
        assert tr.norm_every == 1                                    # the logger's cadence wins
        (opt,) = tr.opts
        for step in range(2):                                        # the learning rate of step 0 is 0 (warm-up): nothing moves there
            tr.train_step({"image": torch.from_numpy(train_step_s2_batch(step)).to(dev)}, step)
        (stats,) = tr.norm_stats()
        lg.close()
    assert len(stats) == len(opt.flat.params) and set(stats) <= {n for n, _ in model.named_parameters()}
    for n, e in stats.items():
        assert all(np.isfinite(e[k]) for k in ("grad_norm", "grad_absmax", "weight_norm", "update_norm", "update_ratio")), n
    assert sum(e["grad_norm"] > 0 for e in stats.values()) > len(stats) // 2
    row = tr.norm_tracker.last_row
    assert row[0] == 1 and row[1]["grad_2.0_norm_total_opt0"] > 0 and row[1]["grad_nonfinite_opt0"] == 0
    import csv
    with open(tmp_path / "metrics.csv", newline="") as f:
        first, mrow = [r for r in csv.DictReader(f) if r.get("grad_2.0_norm_total_opt0")]
    assert float(first["update_ratio_total_opt0"]) == 0.0 and first["step"] == "0" and mrow["step"] == "1"
    assert mrow["grad_2.0_norm_total_opt0"] == repr(row[1]["grad_2.0_norm_total_opt0"]) and mrow["grad_nonfinite_opt0"] == "0"
    assert float(mrow["update_ratio_max_opt0"]) >= float(mrow["update_ratio_total_opt0"]) > 0 and float(mrow["weight_norm_total_opt0"]) > 0
    with open(tmp_path / "norms.csv", newline="") as f:
        groups = [r["name"] for r in csv.DictReader(f) if r["step"] == "1"]
    assert groups == list(dict.fromkeys(".".join(n.split(".")[:2]) for n in stats)) and len(groups) < len(stats)
    (ev,) = os.listdir(tmp_path / "tensorboard")
    data = open(tmp_path / "tensorboard" / ev, "rb").read()
    assert f"norms/grad_norm/opt0.{groups[0]}".encode() in data and b"norms/update_ratio/opt0." in data
