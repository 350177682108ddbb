"""Host side of per-parameter norm tracking (docs/design/24-norm-tracking.md): command-line flags, Trainer arguments, prefix grouping
and fp64 aggregation, norms.csv, the metrics row's keys, the library's exports and host-side argument checks.  No GPU needed."""
import csv
import ctypes as C
import inspect
import math
import os
import sys

import numpy as np
import pytest

from conftest import REPO

import normtrack_math as NM


def _train():
    sys.path.insert(0, REPO)
    import train
    return train


def test_flags_parse_and_default_off():
    train = _train()
    p = train.get_parser()
    opt, unknown = p.parse_known_args(["-b", "x.yml"])
    assert opt.track_grad_norm == "-1" and opt.track_norm_depth == 0 and opt.no_track_updates is False and unknown == []
    opt, unknown = p.parse_known_args(["-b", "x.yml", "--track_grad_norm", "2", "--track_norm_depth", "3", "--no_track_updates",
                                       "--accumulate_grad_batches", "2"])
    assert opt.track_grad_norm == "2" and opt.track_norm_depth == 3 and opt.no_track_updates is True
    dot, ignored = train.split_unknown(unknown)
    assert dot == [] and ignored == ["--accumulate_grad_batches", "2"]
    opt, _ = p.parse_known_args(["-b", "x.yml", "--track_grad_norm", "inf"])
    assert opt.track_grad_norm == "inf"
    with pytest.raises(SystemExit):
        p.parse_known_args(["-b", "x.yml", "--track_grad_norm", "3"])


def test_track_grad_norm_values():
    from dynamicvectorquantization_amd.normtrack import parse_track_grad_norm, total_key
    assert parse_track_grad_norm(-1) == -1 and parse_track_grad_norm("-1") == -1
    assert parse_track_grad_norm(2) == 2 and parse_track_grad_norm("2") == 2 and parse_track_grad_norm(2.0) == 2
    assert parse_track_grad_norm("inf") == "inf" and parse_track_grad_norm(float("inf")) == "inf"
    for bad in (0, 1, 3, "l2", None, True, float("nan")):
        with pytest.raises(ValueError):
            parse_track_grad_norm(bad)
    assert total_key(2) == "grad_2.0_norm_total" and total_key("inf") == "grad_inf_norm_total"


def test_flags_round_trip_through_the_saved_config():
    from dynamicvectorquantization_amd import config as cfg
    base = cfg.load_yaml(os.path.join(REPO, "configs/stage1/dqvae-entropy-dual-r05_imagenet.yml"))
    merged = cfg.merge(base, {"lightning": {"trainer": {"track_grad_norm": "inf", "track_norm_depth": 2, "track_updates": False,
                                                        "log_every_n_steps": 7}}})
    plain = cfg.to_plain(merged)
    assert plain["lightning"]["trainer"] == {"track_grad_norm": "inf", "track_norm_depth": 2, "track_updates": False, "log_every_n_steps": 7}
    assert plain["model"] == cfg.to_plain(base)["model"]
    import yaml
    back = yaml.safe_load(yaml.safe_dump(plain))["lightning"]["trainer"]
    assert str(back["track_grad_norm"]) == "inf" and back["track_norm_depth"] == 2 and back["track_updates"] is False
    src = open(os.path.join(REPO, "train.py")).read()
    assert '"track_grad_norm": opt.track_grad_norm' in src and "track_grad_norm=track_grad_norm" in src
    assert 'saved_trainer.get("track_grad_norm"' in src and 'saved_trainer.get("track_norm_depth"' in src


def test_trainer_signature_carries_track_grad_norm_off():
    from dynamicvectorquantization_amd.trainer import HipAdam, Trainer
    par = inspect.signature(Trainer.__init__).parameters
    assert par["track_grad_norm"].default == -1 and par["track_updates"].default is True and "norm_every" in par
    assert hasattr(Trainer, "norm_stats") and hasattr(HipAdam, "set_norm_tracking") and hasattr(HipAdam, "norm_stats")
    par = inspect.signature(HipAdam.set_norm_tracking).parameters
    assert list(par)[1:] == ["names", "track_updates"] and par["track_updates"].default is True


def _entry(numel, g, gmax, bad, w, u):
    return {"numel": numel, "grad_norm": g, "grad_absmax": gmax, "grad_nonfinite": bad, "grad_nonfinite_total": bad, "first_bad_step": 4 if bad else -1,
            "weight_norm": w, "update_norm": u, "update_ratio": None if u is None else (u / w if w else 0.0)}


STATS = {"encoder.down.0.weight": _entry(10, 3.0, 2.5, 0, 6.0, 0.375),
         "encoder.down.0.bias": _entry(2, 4.0, 3.5, 1, 8.0, 0.5),
         "encoder.mid.weight": _entry(5, 12.0, 9.0, 0, 0.0, 0.0),
         "decoder.out.weight": _entry(7, 2.0 ** -10, 2.0 ** -10, 2, 2.0, 1.0),
         "logit_scale": _entry(1, 0.5, 0.5, 0, 1.0, 1e-4)}


def test_prefix_grouping_aggregates_in_fp64():
    from dynamicvectorquantization_amd.normtrack import group_stats, totals
    assert group_stats(STATS, 0).keys() == STATS.keys()
    flat = group_stats(STATS, 0)["encoder.down.0.bias"]
    assert flat == {"numel": 2, "grad_norm": 4.0, "grad_absmax": 3.5, "grad_nonfinite": 1, "weight_norm": 8.0, "update_norm": 0.5, "update_ratio": 0.5 / 8.0}
    g1 = group_stats(STATS, 1)
    assert list(g1) == ["encoder", "decoder", "logit_scale"]
    assert g1["encoder"]["numel"] == 17 and g1["encoder"]["grad_norm"] == 13.0 and g1["encoder"]["grad_absmax"] == 9.0
    assert g1["encoder"]["grad_nonfinite"] == 1 and g1["encoder"]["weight_norm"] == 10.0 and g1["encoder"]["update_norm"] == 0.625
    assert g1["encoder"]["update_ratio"] == 0.625 / 10.0
    g2 = group_stats(STATS, 2)
    assert list(g2) == ["encoder.down", "encoder.mid", "decoder.out", "logit_scale"]
    assert g2["encoder.down"]["grad_norm"] == 5.0 and g2["encoder.mid"]["update_ratio"] == 0.0          # 0 / 0: nothing moved
    for depth in (1, 2, 5):
        want = NM.group(STATS, depth)
        got = group_stats(STATS, depth)
        assert list(got) == list(want)
        for k, w in want.items():
            assert got[k]["numel"] == w["numel"] and got[k]["grad_nonfinite"] == w["bad"] and got[k]["grad_absmax"] == w["absmax"]
            assert got[k]["grad_norm"] == math.sqrt(w["g2"]) and got[k]["weight_norm"] == math.sqrt(w["w2"]) and got[k]["update_norm"] == math.sqrt(w["u2"])
    t = totals(STATS, 2)
    assert t["grad_total"] == math.sqrt(9 + 16 + 144 + 2.0 ** -20 + 0.25) and t["grad_nonfinite"] == 3
    assert t["weight_norm_total"] == math.sqrt(36 + 64 + 0 + 4 + 1) and t["update_ratio_max"] == 0.5
    assert totals(STATS, "inf")["grad_total"] == 9.0
    no_updates = {n: {**e, "update_norm": None, "update_ratio": None} for n, e in STATS.items()}
    assert group_stats(no_updates, 1)["encoder"]["update_norm"] is None and totals(no_updates)["update_ratio_max"] is None


def test_metric_row_keys():
    from dynamicvectorquantization_amd.normtrack import metric_row
    row = metric_row([STATS, None, STATS], 2)
    assert sorted(row) == sorted([f"{k}_opt{i}" for i in (0, 2) for k in ("grad_2.0_norm_total", "weight_norm_total", "update_ratio_total",
                                                                          "update_ratio_max", "grad_nonfinite")])
    assert "grad_inf_norm_total_opt0" in metric_row([STATS], "inf") and metric_row([STATS], "inf")["grad_inf_norm_total_opt0"] == 9.0
    src = open(os.path.join(REPO, "dynamicvectorquantization_amd", "metrics.py")).read()
    assert "norm_tracker" in src


def test_norms_csv_header_append_and_cells(tmp_path, capsys):
    from dynamicvectorquantization_amd.normtrack import COLUMNS, NormTracker
    assert ",".join(COLUMNS) == "step,epoch,opt,name,numel,grad_norm,grad_absmax,grad_nonfinite,weight_norm,update_norm,update_ratio"
    d = str(tmp_path / "run")
    nt = NormTracker(2, 0, d)
    extra = nt.row(49, 0, [STATS, STATS])
    assert nt.last_row == (49, extra) and extra["grad_nonfinite_opt1"] == 3
    out = capsys.readouterr().out.strip().splitlines()
    assert len(out) == 2 and out[0].startswith("[norms] opt0") and "encoder.down.0.bias (1 elements, first at step 4)" in out[0]
    nt.row(99, 1, [STATS, STATS])
    assert capsys.readouterr().out == ""                              # the running totals have not grown: said once
    NormTracker(2, 1, d).row(149, 1, [STATS], report=None)            # a resumed run: appended, the header kept; grouped by one component
    with open(os.path.join(d, "norms.csv"), newline="") as f:
        lines = list(csv.reader(f))
    assert lines[0] == list(COLUMNS) and sum(l == list(COLUMNS) for l in lines) == 1
    assert len(lines) == 1 + 2 * 2 * len(STATS) + 3
    first = dict(zip(COLUMNS, lines[1]))
    assert first == {"step": "49", "epoch": "0", "opt": "0", "name": "encoder.down.0.weight", "numel": "10", "grad_norm": repr(3.0), "grad_absmax": repr(2.5),
                     "grad_nonfinite": "0", "weight_norm": repr(6.0), "update_norm": repr(0.375), "update_ratio": repr(0.375 / 6.0)}
    for l in lines[1:]:
        for cell in l[5:7] + l[8:]:
            assert cell == repr(float(cell))
    last = dict(zip(COLUMNS, lines[-1]))
    assert last["step"] == "149" and last["name"] == "logit_scale" and dict(zip(COLUMNS, lines[-3]))["name"] == "encoder"
    many = {f"p{i}": _entry(1, 1.0, 1.0, 1, 1.0, 0.1) for i in range(8)}
    NormTracker(2, 0, None).row(0, 0, [many])
    line = capsys.readouterr().out.strip()
    assert line.count("elements, first at step") == 5 and line.endswith("and 3 more")
    assert not os.path.exists(os.path.join(str(tmp_path), "norms.csv"))


def test_tensorboard_scalars_at_the_chosen_depth(tmp_path):
    from dynamicvectorquantization_amd.normtrack import NormTracker

    class Rec:
        def write(self, row, epoch, step):
            self.args = (row, epoch, step)
    rec = Rec()
    NormTracker("inf", 1, None).row(9, 0, [STATS], tensorboard=rec, report=None)
    row, epoch, step = rec.args
    assert (epoch, step) == (0, 9) and row["norms/grad_norm/opt0.encoder"] == 13.0 and row["norms/update_ratio/opt0.decoder"] == 0.5
    assert len(row) == 5 * 3


def test_library_exports_the_segment_kernels():
    from dynamicvectorquantization_amd import _lib, build
    build.build(verbose=False)
    lib = _lib.load()
    assert "normtrack.hip" in build.SOURCES
    for n in ("dvq_segment_stats", "dvq_segment_stats_workspace_bytes", "dvq_segment_stats_state_bytes", "dvq_segment_plan_bytes",
              "dvq_segment_plan_build", "dvq_copy_f32_armed"):
        assert n in _lib.SIGNATURES and hasattr(lib, n)
    assert lib.dvq_version() == 124
    from dynamicvectorquantization_amd import kernels as K
    c = K.GRAD_SQNORM_CHUNK                                          # one chunk length for both reductions
    assert lib.dvq_grad_sqnorm_workspace_bytes(c) == 8 and lib.dvq_grad_sqnorm_workspace_bytes(c + 1) == 16
    assert lib.dvq_segment_stats_state_bytes(1) == 48 and lib.dvq_segment_stats_state_bytes(2) == 88 and lib.dvq_segment_stats_state_bytes(0) == 0
    assert lib.dvq_segment_stats_workspace_bytes(3 * c + 5, 4) == 16 * 7 and lib.dvq_segment_stats_workspace_bytes(3, 4) == 0
    # the plan is built on the host: segment lengths around the chunk, checked against the restatement of the table
    lengths = [1, c - 1, c, c + 1, 2 * c + 7, 2]
    offs = NM.offsets_of(lengths)
    arr = (C.c_int64 * len(offs))(*[int(v) for v in offs])
    S, n = len(lengths), int(offs[-1])
    nbytes = lib.dvq_segment_plan_bytes(arr, S, n)
    nchunks = sum(-(-l // c) for l in lengths)
    assert nchunks == 9 and nbytes == 32 + 2 * 8 * (S + 1) + 16 * nchunks
    plan = np.zeros(nbytes // 8, np.int64)
    assert lib.dvq_segment_plan_build(arr, S, n, plan.ctypes.data, nbytes) == 0
    assert list(plan[:4]) == [n, S, nchunks, c] and np.array_equal(plan[4:5 + S], offs)
    chunk0 = plan[5 + S:6 + 2 * S]
    assert list(chunk0) == [0, 1, 2, 3, 5, 8, 9]
    table = plan[6 + 2 * S:].reshape(nchunks, 2)
    starts, seg, ln = table[:, 0], table[:, 1] & 0xFFFFFFFF, table[:, 1] >> 32
    want = [(int(offs[s]) + k * c, s, min(c, lengths[s] - k * c)) for s in range(S) for k in range(-(-lengths[s] // c))]
    assert [(int(a), int(b), int(d)) for a, b, d in zip(starts, seg, ln)] == want
    assert lib.dvq_segment_plan_build(arr, S, n, plan.ctypes.data, nbytes - 8) == -1
    # argument checks come before any launch: they answer without a GPU
    bad = (C.c_int64 * len(offs))(*[int(v) for v in offs])
    bad[2], bad[3] = bad[3], bad[2]
    assert lib.dvq_segment_plan_bytes(bad, S, n) == 0 and lib.dvq_segment_plan_build(bad, S, n, plan.ctypes.data, nbytes) == -2
    assert lib.dvq_segment_plan_bytes(arr, S, n + 1) == 0 and lib.dvq_segment_plan_bytes(arr, S - 1, n) == 0
    fake = C.c_void_p(1 << 20)
    assert lib.dvq_segment_stats(fake, None, n, bad, S, fake, nbytes, fake, 1 << 20, fake, 0, None, None) == -2         # DVQ_ESHAPE
    assert lib.dvq_segment_stats(fake, None, n, arr, S, fake, nbytes + 16, fake, 1 << 20, fake, 0, None, None) == -2
    assert lib.dvq_segment_stats(fake, None, n, arr, S, fake, nbytes, fake, 16 * nchunks - 1, fake, 0, None, None) == -5      # DVQ_EWORKSPACE
    assert lib.dvq_segment_stats(None, None, n, arr, S, fake, nbytes, fake, 1 << 20, fake, 0, None, None) == -1
    assert lib.dvq_copy_f32_armed(None, fake, 4, None, None) == -1 and lib.dvq_copy_f32_armed(fake, fake, 0, None, None) == -1
    header = open(os.path.join(REPO, "include", "dvq_hip.h")).read()
    assert "int dvq_copy_f32_armed(float* dst, const float* src, int64_t n, const int* armed, dvq_stream_t stream);" in header
