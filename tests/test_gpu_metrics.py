"""Training metric logs on the GPU (csrc/trainlog.hip, metrics.py, Trainer(metrics_logger=...); docs/design/22-metrics-logging.md).
`pytest -m gpu`.  The kernels against tests/trainlog_math.py, the trainer against a second, identically seeded run that reads the
model's logged tensors on the host."""
import csv
import ctypes
import os

import numpy as np
import pytest
import torch

import trainlog_math as TM
from dynamicvectorquantization_amd import synth

pytestmark = pytest.mark.gpu

TORCH_T = {TM.F32: torch.float32, TM.BF16: torch.bfloat16, TM.F64: torch.float64, TM.I32: torch.int32, TM.I64: torch.int64}
FLOATING = (TM.F32, TM.BF16, TM.F64, TM.IMM)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


# ---- dvq_scalar_push -------------------------------------------------------------------------------------------------------------------
def _push_case(k, seed=0):
    """type code per column and five pushes of host values (already of the column's type) with a NaN, two Infs, an fp64 value beyond
    fp32's range and, from two columns on, columns that sit a push out"""
    rs = np.random.RandomState(100 * k + seed)
    codes = [TM.F32] if k == 1 else [c % 6 for c in range(k)]
    pushes = []
    for _ in range(5):
        vals = []
        for code in codes:
            if code == TM.I32:
                v = int(rs.randint(-2 ** 31, 2 ** 31 - 1))
            elif code == TM.I64:
                v = int(rs.randint(-2 ** 31, 2 ** 31 - 1)) * 2 ** 29 + int(rs.randint(0, 2 ** 29))
            else:
                v = rs.standard_normal() * 10.0 ** rs.uniform(-3, 6)
            vals.append(TM.typed(code, v))
        pushes.append(vals)
    fl = [c for c, code in enumerate(codes) if code in FLOATING]
    pushes[1][fl[0]] = TM.typed(codes[fl[0]], float("nan"))
    pushes[3][fl[-1]] = TM.typed(codes[fl[-1]], float("-inf"))
    pushes[2][fl[len(fl) // 2]] = TM.typed(codes[fl[len(fl) // 2]], float("inf"))
    f64 = [c for c, code in enumerate(codes) if code == TM.F64]
    if f64:
        pushes[4][f64[0]] = np.float64(1e300)                # finite: counted and summed; its fp32 cast is +Inf
    skipped = []
    for p in range(5):
        sk = [c for c in range(k) if k > 1 and p == 2 and c % 7 == 3]
        skipped.append(sk)
    return codes, pushes, skipped


def _device_values(dev, codes, vals, skip):
    """one device array per element type (one upload each); a column's value is a one-element view of its type's array"""
    slots = [None] * len(codes)
    for code, tt in TORCH_T.items():
        cols = [c for c, cc in enumerate(codes) if cc == code and c not in skip]
        if not cols:
            continue
        host = np.array([vals[c] for c in cols], dtype={TM.F32: np.float32, TM.BF16: np.float32, TM.F64: np.float64, TM.I32: np.int32,
                                                        TM.I64: np.int64}[code])
        arr = torch.from_numpy(host).to(dev)
        if code == TM.BF16:
            arr = arr.to(torch.bfloat16)                     # exact: the values are bf16-representable
        for j, c in enumerate(cols):
            slots[c] = arr[j:j + 1]
    for c, cc in enumerate(codes):
        if cc == TM.IMM and c not in skip:
            slots[c] = float(vals[c])
    return slots


def _run_pushes(dev, k, codes, pushes, skipped):
    from dynamicvectorquantization_amd import kernels as K
    state = K.scalar_push_state(k, dev)
    keep = []
    for vals, sk in zip(pushes, skipped):
        slots = _device_values(dev, codes, vals, sk)
        keep.append(slots)
        K.scalar_push(slots, state, k)
    torch.cuda.synchronize()
    return state.cpu()


@pytest.mark.parametrize("k", [1, 64, 65, 256])
def test_scalar_push_matches_the_sequential_restatement(dev, k):
    """last = the fp32 cast bit for bit; sum / cnt / bad = the sequential fp64 restatement bit for bit (one owner per column, the order
    of the launches); two identical sequences leave identical state; the unordered-launch counter does not move"""
    from dynamicvectorquantization_amd import kernels as K
    codes, pushes, skipped = _push_case(k)
    ref = TM.new_state(k)
    for vals, sk in zip(pushes, skipped):
        TM.scalar_push(ref, [TM.SKIP if c in sk else code for c, code in enumerate(codes)], vals)
    assert int(ref["bad"].sum()) >= 2 and int((ref["cnt"] + ref["bad"]).sum()) == 5 * k - sum(len(s) for s in skipped)
    c0 = K.unordered_launches()
    a = _run_pushes(dev, k, codes, pushes, skipped)
    b = _run_pushes(dev, k, codes, pushes, skipped)
    assert K.unordered_launches() == c0
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    s, cnt, bad, last = (t.numpy() for t in K.scalar_push_views(a, k))
    assert np.array_equal(_bits(last), _bits(ref["last"]))
    assert np.array_equal(_bits(s), _bits(ref["sum"]))
    assert np.array_equal(cnt, ref["cnt"]) and np.array_equal(bad, ref["bad"])


def test_scalar_push_refuses_more_than_256_columns(dev):
    from dynamicvectorquantization_amd import _lib
    from dynamicvectorquantization_amd import kernels as K
    lib = _lib.load()
    state = K.scalar_push_state(256, dev)
    one = torch.ones(1, device=dev)
    rec = _lib.ScalarRecord()
    rec.addr[0], rec.code[0] = one.data_ptr(), _lib.SCALAR_F32
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert lib.dvq_scalar_push(ctypes.byref(rec), 1, 256, 257, ctypes.c_void_p(state.data_ptr()), stream) == -2       # DVQ_ESHAPE
    assert lib.dvq_scalar_push_state_bytes(257) == 0
    with pytest.raises(_lib.DvqError):
        K.scalar_push_state(257, dev)
    with pytest.raises(_lib.DvqError):
        K.scalar_push([1.0] * 257, state, 256)
    torch.cuda.synchronize()
    assert not state.any()                                   # nothing was launched


# ---- dvq_codebook_health ---------------------------------------------------------------------------------------------------------------
def _counts(pattern, k, kind, rs):
    hi = 2 ** 40 if kind == "int64" else 2 ** 12               # fp32 counts are whole numbers far below 2^24
    if pattern == "zeros":
        n = np.zeros(k, np.int64)
    elif pattern == "onehot":
        n = np.zeros(k, np.int64)
        n[(3 * k) // 4] = 37
    elif pattern == "uniform":
        n = np.full(k, 5, np.int64)
    else:
        n = rs.randint(1, hi, size=k).astype(np.int64)
        if k > 1:
            n[rs.rand(k) < 0.3] = 0
    return n


@pytest.mark.parametrize("kind", ["fp32-strided", "int64"])
@pytest.mark.parametrize("k", [1, 1000, 1024])
def test_codebook_health_matches_fp64(dev, k, kind):
    """perplexity / active codes / tokens: 1e-9 relative on the fp64 values (K <= 16384 terms at 2^-53 each, times a few ulp of log: below
    1e-11, the margin covers a different log), the fp32 outputs = those values rounded, within 1 ulp of the rounded reference; the
    running total exact (whole numbers below 2^53)"""
    from dynamicvectorquantization_amd import kernels as K
    rs = np.random.RandomState(k)
    d = 7
    for pattern in ("random", "zeros", "onehot", "uniform"):
        n = _counts(pattern, k, kind, rs)
        if kind == "int64":
            counts, stride = torch.from_numpy(n).to(dev), 1
        else:
            stats = torch.full((k, d + 1), float("nan"), device=dev)          # only column D may be read
            stats[:, d] = torch.from_numpy(n.astype(np.float32)).to(dev)
            counts, stride = stats[:, d], d + 1
        out3 = torch.full((3,), -1.0, device=dev)
        out64 = torch.full((3,), -1.0, dtype=torch.float64, device=dev)
        total = torch.zeros(k, dtype=torch.float64, device=dev)
        K.codebook_health(counts, k, stride, out3, total=total, out3_f64=out64)
        first = out64.clone()
        K.codebook_health(counts, k, stride, out3, total=total, out3_f64=out64)
        torch.cuda.synchronize()
        assert torch.equal(first.view(torch.int64), out64.view(torch.int64)), pattern
        ref = np.array(TM.codebook_health(n), np.float64)
        got64, got32 = out64.cpu().numpy(), out3.cpu().numpy()
        print(f"codebook_health {kind} K={k} {pattern}: got {got64.tolist()} ref {ref.tolist()}")
        assert np.all(np.abs(got64 - ref) <= 1e-9 * np.abs(ref)), (pattern, got64, ref)
        assert np.array_equal(_bits(got32), _bits(got64.astype(np.float32))), pattern
        assert np.all(np.abs(_bits(got32).astype(np.int64) - _bits(ref.astype(np.float32)).astype(np.int64)) <= 1), pattern
        assert np.array_equal(total.cpu().numpy(), 2.0 * n.astype(np.float64)), pattern
        if pattern == "zeros":
            assert got64.tolist() == [0.0, 0.0, 0.0]
        if pattern == "onehot":
            assert got64.tolist() == [1.0, 1.0, 37.0]
        if pattern == "uniform":
            assert abs(got64[0] - k) <= 1e-9 * k and got64[1] == k and got64[2] == 5.0 * k


# ---- Trainer, stage 1 ------------------------------------------------------------------------------------------------------------------
def _rows(logdir):
    with open(os.path.join(logdir, "metrics.csv"), newline="") as f:
        return list(csv.DictReader(f))


def _stage1_run(dev, logdir, steps=12, bs=4):
    """the `small` stage-1 model with the shipped two-optimizer objective under Trainer(deterministic=True, graph_after=3): steps 0-2
    eager, step 3 recorded and replayed, 4-11 replayed.  logdir None: no logger, the logged tensors read on the host after every step"""
    from dynamicvectorquantization_amd import kernels as K
    from dynamicvectorquantization_amd import runtime as rt
    from dynamicvectorquantization_amd.config import instantiate_from_config
    from dynamicvectorquantization_amd.metrics import MetricsLogger
    from dynamicvectorquantization_amd.trainer import Trainer
    from golden_cfg import TRAIN_STEP
    from test_gpu_model import GEOM, model_config
    c, g = TRAIN_STEP["small"], GEOM["small"]
    out = {"reads": [], "losses": []}
    try:
        with rt.compute_dtype_ctx("fp32"):
            torch.manual_seed(0)
            model = instantiate_from_config(model_config(**g, loss="full", ndf=c["ndf"])).to(dev)
            synth.apply_train_step_state(model, g["k"], g["zc"])
            rt.bump_weights_epoch()
            model.learning_rate, model.min_learning_rate = c["lr"], c["min_lr"]
            model.warmup_epochs, model.steps_per_epoch, model.training_steps = c["warmup_epochs"], 6, c["training_steps"]
            model.train()
            lg = MetricsLogger(logdir, writers=("csv", "tensorboard"), log_every_n_steps=4) if logdir else None
            tr = Trainer(model, max_steps=steps, use_graph=True, graph_after=3, deterministic=True, metrics_logger=lg)
            for step, xb in enumerate(synth.train_step_batches(steps, bs, g["resolution"])):
                losses = tr.train_step({"image": torch.from_numpy(xb).to(dev)}, step)
                if lg is None:
                    out["reads"].append({k: float(v.detach() if torch.is_tensor(v) else v) for k, v in model._logged.items()})
                out["losses"].append([float(l) for l in losses])
            if lg is not None:
                lg.finish(tr)
            torch.cuda.synchronize()
            assert tr.use_graph and tr.graph_replays == steps - 3, (tr.use_graph, tr.graph_replays)
            out["params"] = [o.flat.flat_p.clone() for o in tr.opts]
            out["tokens"] = int(model._last["codes"].numel())
    finally:
        K.set_deterministic(False)
    return out


@pytest.fixture(scope="module")
def stage1_runs(dev, tmp_path_factory):
    logdir = str(tmp_path_factory.mktemp("stage1_metrics"))
    return logdir, _stage1_run(dev, logdir), _stage1_run(dev, None)


def test_stage1_step_rows_equal_host_reads(stage1_runs):
    """eager, recorded and replayed steps: every `_step` cell at steps 3, 7, 11 has the float32 bits of float(model._logged[k]) read
    after that step in the run without a logger"""
    logdir, _, plain = stage1_runs
    rows = [r for r in _rows(logdir) if r["train_aeloss_step"] != ""]
    assert [int(r["step"]) for r in rows] == [3, 7, 11] and [int(r["epoch"]) for r in rows] == [0, 1, 1]
    for r in rows:
        reads = plain["reads"][int(r["step"])]
        logged = {k[:-5] for k, v in r.items() if k.endswith("_step") and v != "" and not k.startswith("train_codebook_")}
        assert logged == set(reads) and len(logged) >= 10, logged ^ set(reads)
        for k, v in reads.items():
            assert np.float32(float(r[k + "_step"])).tobytes() == np.float32(v).tobytes(), (r["step"], k, r[k + "_step"], v)
        assert float(r["lr_opt0"]) > 0 and float(r["lr_opt1"]) > 0 and float(r["images_per_sec"]) > 0
    assert len({r["train_aeloss_step"] for r in rows}) == 3 and len({r["train_discloss_step"] for r in rows}) == 3      # no stale pointer


def test_stage1_epoch_rows_are_fp64_means(stage1_runs):
    logdir, _, plain = stage1_runs
    rows = [r for r in _rows(logdir) if r["train_aeloss_epoch"] != ""]
    assert [int(r["step"]) for r in rows] == [5, 11] and [int(r["epoch"]) for r in rows] == [0, 1]
    for e, r in enumerate(rows):
        for k in plain["reads"][0]:
            s = np.float64(0.0)
            for step in range(6 * e, 6 * e + 6):
                s = s + np.float64(plain["reads"][step][k])
            assert float(r[k + "_epoch"]) == float(s / 6), (e, k)
        assert r.get("nonfinite_values_epoch", "") == ""


def test_stage1_codebook_keys(stage1_runs):
    logdir, run, _ = stage1_runs
    rows = _rows(logdir)
    steps = [r for r in rows if r["train_aeloss_step"] != ""]
    assert run["tokens"] == 4 * 8 * 8
    for r in steps:
        assert float(r["train_codebook_tokens_step"]) == run["tokens"]
        active, ppl = float(r["train_codebook_active_step"]), float(r["train_codebook_perplexity_step"])
        assert 1 <= active <= 512 and active == int(active) and 1.0 <= ppl <= active * (1 + 1e-6)
    for r in (r for r in rows if r["train_aeloss_epoch"] != ""):
        dead, ppl = int(r["train_codebook_dead_epoch"]), float(r["train_codebook_perplexity_epoch"])
        assert 0 <= dead < 512 and 1.0 <= ppl <= (512 - dead) * (1 + 1e-9)
        assert float(r["train_codebook_tokens_epoch"]) == run["tokens"]


def test_stage1_logger_does_not_disturb_training(stage1_runs):
    _, run, plain = stage1_runs
    assert run["losses"] == plain["losses"]
    for a, b in zip(run["params"], plain["params"]):
        assert torch.equal(a, b)


def test_stage1_event_file_has_the_step_rows(stage1_runs):
    from test_metrics_cpu import read_event_file
    logdir, _, _ = stage1_runs
    d = os.path.join(logdir, "tensorboard")
    (name,) = os.listdir(d)
    version, triples = read_event_file(os.path.join(d, name))
    assert version == "brain.Event:2"
    assert [s for t, s, _ in triples if t == "train_aeloss_step"] == [3, 7, 11]
    assert [s for t, s, _ in triples if t == "train_aeloss_epoch"] == [5, 11]
    rows = {int(r["step"]): r for r in _rows(logdir) if r["train_aeloss_step"] != ""}
    for t, s, v in triples:
        if t == "train_rec_loss_step":
            assert v.tobytes() == np.float32(float(rows[s][t])).tobytes()


# ---- Trainer, stage 2 ------------------------------------------------------------------------------------------------------------------
def test_stage2_rows(dev, tmp_path):
    """the stage-2 model's keys in `_step` and `_epoch` form with lr_opt0; the values move from row to row and equal the step's own
    logged tensors (stage-2 steps are never recorded: every step is eager)"""
    from dynamicvectorquantization_amd import runtime as rt
    from dynamicvectorquantization_amd.config import instantiate_from_config
    from dynamicvectorquantization_amd.metrics import MetricsLogger
    from dynamicvectorquantization_amd.trainer import Trainer
    from test_gpu_stage2 import dualformer_config
    with rt.compute_dtype_ctx(torch.bfloat16):
        torch.manual_seed(0)
        model = instantiate_from_config(dualformer_config()).to(dev)
        model.learning_rate, model.min_learning_rate, model.training_steps, model.steps_per_epoch = 3e-3, 0.0, 100, 3
        model.train()
        x = torch.from_numpy(synth.half_flat_images(4, 64, seed=11)).to(dev)
        lg = MetricsLogger(str(tmp_path), writers=("csv",), log_every_n_steps=2)
        tr = Trainer(model, max_steps=6, metrics_logger=lg)
        reads = []
        for i in range(6):
            tr.train_step({"image": x}, i)
            reads.append({k: float(v.detach() if torch.is_tensor(v) else v) for k, v in model._logged.items()})
        lg.finish(tr)
    rows = _rows(str(tmp_path))
    keys = ("train_loss", "train_content_loss", "train_position_loss")
    steps = [r for r in rows if r["train_loss_step"] != ""]
    assert [int(r["step"]) for r in steps] == [1, 3, 5]
    for r in steps:
        for k in keys + ("train_coarse_position_loss", "train_fine_position_loss"):
            assert np.float32(float(r[k + "_step"])).tobytes() == np.float32(reads[int(r["step"])][k]).tobytes(), k
        assert float(r["lr_opt0"]) > 0
        assert "train_codebook_tokens_step" not in r                 # the frozen first stage updates no codebook
    for k in keys:
        assert len({r[k + "_step"] for r in steps}) == 3, k
    epochs = [r for r in rows if r["train_loss_epoch"] != ""]
    assert [int(r["step"]) for r in epochs] == [2, 5]
    for e, r in enumerate(epochs):
        for k in keys:
            s = np.float64(0.0)
            for i in range(3 * e, 3 * e + 3):
                s = s + np.float64(reads[i][k])
            assert float(r[k + "_epoch"]) == float(s / 3), k


# ---- train.py ----------------------------------------------------------------------------------------------------------------------------
def test_train_py_logger_flags_and_resume(dev, tmp_path):
    """`train.py -l csv,tensorboard,wandb --log_every_n_steps 2` on synthetic batches: both files appear, wandb is named as ignored, the
    flags land in the saved project.yaml, and `-r <logdir>` WITHOUT the flags keeps logging into the same files with the run's step
    numbering"""
    import subprocess
    import sys
    import yaml
    from conftest import REPO
    from test_gpu_model import GEOM, model_config
    mc = model_config(**GEOM["small"], loss="ae")
    mc["base_learning_rate"] = 1e-5
    cfg_path = tmp_path / "tiny.yml"
    yaml.safe_dump({"model": mc, "data": {"params": {"batch_size": 2}}}, open(cfg_path, "w"))
    logs = tmp_path / "logs"
    common = ["--steps_per_epoch", "3", "--max_epochs", "2", "--val_batches", "1"]
    r = subprocess.run([sys.executable, os.path.join(REPO, "train.py"), "-b", str(cfg_path), "-l", "csv,tensorboard,wandb", "--log_every_n_steps", "2",
                        "--max_steps", "4", "--logdir", str(logs), "-n", "m"] + common, cwd=REPO, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert "ignoring unsupported loggers: ['wandb']" in r.stdout
    (run,) = os.listdir(logs)
    logdir = str(logs / run)
    saved = yaml.safe_load(open(os.path.join(logdir, "configs", "project.yaml")))
    assert saved["lightning"]["trainer"] == {"logger": "csv,tensorboard", "log_every_n_steps": 2}
    assert sorted(os.listdir(logdir)) == ["checkpoints", "configs", "metrics.csv", "tensorboard"]
    rows = _rows(logdir)
    assert [int(r_["step"]) for r_ in rows if r_["train_aeloss_step"] != ""] == [1, 3]
    assert [int(r_["step"]) for r_ in rows if r_["train_aeloss_epoch"] != ""] == [2, 3]
    assert [int(r_["step"]) for r_ in rows if r_["val_rec_loss_epoch"] != ""] == [2, 3]
    assert all(float(r_["lr_opt0"]) > 0 and float(r_["train_codebook_tokens_step"]) == 2 * 64 for r_ in rows if r_["train_aeloss_step"] != "")
    first = open(os.path.join(logdir, "metrics.csv")).read()
    r2 = subprocess.run([sys.executable, os.path.join(REPO, "train.py"), "-r", logdir] + common, cwd=REPO, capture_output=True, text=True, timeout=300)
    assert r2.returncode == 0 and "resumed from" in r2.stdout, r2.stdout[-2000:] + r2.stderr[-3000:]
    assert open(os.path.join(logdir, "metrics.csv")).read().startswith(first)
    rows = _rows(logdir)
    assert [int(r_["step"]) for r_ in rows if r_["train_aeloss_step"] != ""] == [1, 3, 5]
    assert [int(r_["step"]) for r_ in rows if r_["train_aeloss_epoch"] != ""] == [2, 3, 5]
    assert len(os.listdir(os.path.join(logdir, "tensorboard"))) == 2


# ---- fit end to end ----------------------------------------------------------------------------------------------------------------------
def _ae_model(dev, seed=0):
    from dynamicvectorquantization_amd.config import instantiate_from_config
    from test_gpu_model import GEOM, model_config
    torch.manual_seed(seed)
    model = instantiate_from_config(model_config(**GEOM["small"], loss="ae")).to(dev)
    model.learning_rate, model.min_learning_rate = 2e-4, 1e-5
    model.training_steps, model.steps_per_epoch, model.warmup_epochs = 12, 4, 1
    return model.train()


def test_fit_writes_validation_rows_and_resumes(dev, tmp_path):
    from dynamicvectorquantization_amd.metrics import MetricsLogger
    from dynamicvectorquantization_amd.trainer import Trainer
    xs = [torch.from_numpy(synth.half_flat_images(2, 64, seed=40 + i)).to(dev) for i in range(3)]
    logdir = str(tmp_path / "run")
    ckpt = os.path.join(logdir, "checkpoints", "last.ckpt")

    def batch_fn(step):
        return {"image": xs[step % 3]}

    def val_fn():
        return [{"image": xs[2]}, {"image": xs[0]}]

    tr = Trainer(_ae_model(dev), max_steps=8, use_graph=True, graph_after=2,
                 metrics_logger=MetricsLogger(logdir, writers=("csv",), log_every_n_steps=2))
    tr.fit(batch_fn, ckpt_path=ckpt, val_fn=val_fn, val_every=4)
    assert sorted(os.listdir(logdir)) == ["checkpoints", "metrics.csv"]
    rows = _rows(logdir)
    val = [r for r in rows if r["val_rec_loss_epoch"] != ""]
    assert [int(r["step"]) for r in val] == [3, 7]
    assert float(val[-1]["val_rec_loss_epoch"]) == tr.last_val_metrics["val_rec_loss"]
    assert all(r["train_aeloss_step"] == "" for r in val)
    assert [int(r["step"]) for r in rows if r["train_aeloss_step"] != ""] == [1, 3, 5, 7]
    assert [int(r["step"]) for r in rows if r["train_aeloss_epoch"] != ""] == [3, 7]
    first = open(os.path.join(logdir, "metrics.csv")).read()
    # resumed: a new process would build all of this again; the rows continue behind the old ones with the step numbering of the run
    tr2 = Trainer(_ae_model(dev, seed=5), max_steps=11, use_graph=True, graph_after=2,
                  metrics_logger=MetricsLogger(logdir, writers=("csv",), log_every_n_steps=2))
    tr2.load_state_dict(torch.load(ckpt, map_location="cpu", weights_only=False))
    tr2.fit(batch_fn, ckpt_path=ckpt)
    assert open(os.path.join(logdir, "metrics.csv")).read().startswith(first)
    rows = _rows(logdir)
    assert [int(r["step"]) for r in rows if r["train_aeloss_step"] != ""] == [1, 3, 5, 7, 9]
    assert [int(r["step"]) for r in rows if r["train_aeloss_epoch"] != ""] == [3, 7, 10]        # the partial last epoch at the end of fit
    # without a logger the directory holds what it always held
    plain = str(tmp_path / "plain")
    Trainer(_ae_model(dev), max_steps=3, use_graph=False).fit(batch_fn, ckpt_path=os.path.join(plain, "checkpoints", "last.ckpt"))
    assert os.listdir(plain) == ["checkpoints"] and os.listdir(os.path.join(plain, "checkpoints")) == ["last.ckpt"]
