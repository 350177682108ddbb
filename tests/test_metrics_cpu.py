"""Host side of the training metric logs (docs/design/22-metrics-logging.md): command-line flags, Trainer argument, CRC-32C, the
TensorBoard event file read back by an independent reader, the CSV layout, the numpy restatement of the kernels.  No GPU needed."""
import csv
import inspect
import os
import struct
import sys

import numpy as np
import pytest

from conftest import REPO

import trainlog_math as TM


def _train():
    sys.path.insert(0, REPO)
    import train
    return train


# ---- flags ---------------------------------------------------------------------------------------------------------------------------
def test_logger_flags_parse_and_default_off():
    train = _train()
    p = train.get_parser()
    opt, unknown = p.parse_known_args(["-b", "x.yml"])
    assert opt.logger == "none" and opt.log_every_n_steps == 50 and unknown == []
    opt, unknown = p.parse_known_args(["-b", "x.yml", "-l", "csv,tensorboard", "--log_every_n_steps", "7", "--accumulate_grad_batches", "2",
                                       "--fast_dev_run"])
    assert opt.logger == "csv,tensorboard" and opt.log_every_n_steps == 7
    dot, ignored = train.split_unknown(unknown)
    assert dot == [] and ignored == ["--accumulate_grad_batches", "2", "--fast_dev_run"]
    assert "--log_every_n_steps" not in ignored


def test_logger_flag_values():
    from dynamicvectorquantization_amd.metrics import parse_logger_flag
    assert parse_logger_flag("none") == ((), [])
    assert parse_logger_flag("") == ((), [])
    assert parse_logger_flag("csv") == (("csv",), [])
    assert parse_logger_flag("tensorboard,csv,csv") == (("tensorboard", "csv"), [])
    assert parse_logger_flag("wandb") == ((), ["wandb"])
    assert parse_logger_flag("wandb,csv") == (("csv",), ["wandb"])
    with pytest.raises(ValueError):
        parse_logger_flag("comet")


def test_flags_round_trip_through_the_saved_config():
    from dynamicvectorquantization_amd import config as cfg
    base = cfg.load_yaml(os.path.join(REPO, "configs/stage1/dqvae-entropy-dual-r05_imagenet.yml"))
    merged = cfg.merge(base, {"lightning": {"trainer": {"logger": "csv,tensorboard", "log_every_n_steps": 7}}})
    plain = cfg.to_plain(merged)
    assert plain["lightning"]["trainer"] == {"logger": "csv,tensorboard", "log_every_n_steps": 7}
    assert plain["model"] == cfg.to_plain(base)["model"]
    src = open(os.path.join(REPO, "train.py")).read()
    assert '"logger": ",".join(writers)' in src and "metrics_logger=metrics_logger" in src


def test_trainer_signature_carries_metrics_logger_none():
    from dynamicvectorquantization_amd.trainer import Trainer
    par = inspect.signature(Trainer.__init__).parameters
    assert "metrics_logger" in par and par["metrics_logger"].default is None
    assert "deterministic" in par and par["deterministic"].default is False


def test_library_exports_the_log_kernels():
    from dynamicvectorquantization_amd import _lib, build
    build.build(verbose=False)
    lib = _lib.load()
    assert "trainlog.hip" in build.SOURCES
    for n in ("dvq_scalar_push", "dvq_scalar_push_state_bytes", "dvq_codebook_health"):
        assert n in _lib.SIGNATURES and hasattr(lib, n)
    assert lib.dvq_version() >= 119
    assert lib.dvq_scalar_push_state_bytes(256) == 256 * 28 and lib.dvq_scalar_push_state_bytes(1) == 28
    assert lib.dvq_scalar_push_state_bytes(257) == 0 and lib.dvq_scalar_push_state_bytes(0) == 0
    import ctypes
    assert ctypes.sizeof(_lib.ScalarRecord) == 576
    # argument checks come before any launch: they answer without a GPU
    rec = _lib.ScalarRecord()
    state = (ctypes.c_double * (257 * 4))()
    assert lib.dvq_scalar_push(ctypes.byref(rec), 1, 256, 257, state, None) == -2          # DVQ_ESHAPE: 257 columns
    assert lib.dvq_scalar_push(ctypes.byref(rec), 65, 0, 256, state, None) == -2
    assert lib.dvq_scalar_push(ctypes.byref(rec), 2, 255, 256, state, None) == -2
    assert lib.dvq_scalar_push(ctypes.byref(rec), 1, 0, 256, state, None) == -1            # a null address with a pointer type code


# ---- CRC-32C, TFRecord, Event ----------------------------------------------------------------------------------------------------------
def test_crc32c_known_answers():
    from dynamicvectorquantization_amd.metrics import crc32c, masked_crc32c
    assert crc32c(b"123456789") == 0xE3069283
    assert crc32c(b"") == 0
    assert crc32c(bytes(32)) == 0x8A9136AA                       # RFC 3720 B.4: 32 bytes of zeros
    c = 0xE3069283
    assert masked_crc32c(b"123456789") == ((c >> 15 | c << 17) + 0xA282EAD8) % (1 << 32)


def _crc32c_bitwise(data):
    """independent of the writer's table: the bit-at-a-time definition"""
    c = 0xFFFFFFFF
    for b in data:
        c ^= b
        for _ in range(8):
            c = (c >> 1) ^ (0x82F63B78 & -(c & 1))
    return c ^ 0xFFFFFFFF


def _mask(c):
    return ((c >> 15 | c << 17) + 0xA282EAD8) & 0xFFFFFFFF


def _read_varint(buf, i):
    n, shift = 0, 0
    while True:
        b = buf[i]
        i += 1
        n |= (b & 0x7F) << shift
        shift += 7
        if not b & 0x80:
            return n, i


def _walk(buf):
    """protobuf wire walk -> [(field number, wire type, value)]"""
    out, i = [], 0
    while i < len(buf):
        key, i = _read_varint(buf, i)
        num, wt = key >> 3, key & 7
        if wt == 0:
            v, i = _read_varint(buf, i)
        elif wt == 1:
            v, i = buf[i:i + 8], i + 8
        elif wt == 2:
            n, i = _read_varint(buf, i)
            v, i = buf[i:i + n], i + n
        elif wt == 5:
            v, i = buf[i:i + 4], i + 4
        else:
            raise AssertionError(f"wire type {wt}")
        out.append((num, wt, v))
    assert i == len(buf)
    return out


def read_event_file(path):
    """-> (file_version of the first record, [(tag, step, float32 value)]): TFRecord framing with both checksums verified, then the
    Event / Summary / Value fields"""
    data = open(path, "rb").read()
    i, version, triples, first = 0, None, [], True
    while i < len(data):
        (n,) = struct.unpack_from("<Q", data, i)
        (hc,) = struct.unpack_from("<I", data, i + 8)
        assert hc == _mask(_crc32c_bitwise(data[i:i + 8])), "length checksum"
        payload = data[i + 12:i + 12 + n]
        assert len(payload) == n
        (pc,) = struct.unpack_from("<I", data, i + 12 + n)
        assert pc == _mask(_crc32c_bitwise(payload)), "payload checksum"
        i += 16 + n
        fields = _walk(payload)
        step = next((v for num, wt, v in fields if num == 2 and wt == 0), 0)
        wall = [struct.unpack("<d", v)[0] for num, wt, v in fields if num == 1 and wt == 1]
        assert len(wall) == 1 and wall[0] > 1e9
        if first:
            (version,) = [v.decode() for num, wt, v in fields if num == 3 and wt == 2]
            first = False
            continue
        for num, wt, v in fields:
            if num == 5 and wt == 2:
                for vnum, vwt, val in _walk(v):
                    assert vnum == 1 and vwt == 2
                    inner = _walk(val)
                    (tag,) = [x.decode() for a, b, x in inner if a == 1 and b == 2]
                    (sv,) = [np.frombuffer(x, "<f4")[0] for a, b, x in inner if a == 2 and b == 5]
                    triples.append((tag, step, sv))
    return version, triples


def test_tensorboard_event_file_round_trip(tmp_path):
    from dynamicvectorquantization_amd.metrics import TensorBoardWriter
    w = TensorBoardWriter(str(tmp_path))
    rows = [({"train_loss_step": 0.1, "lr_opt0": 2e-4}, 0, 3),
            ({"train_loss_step": float("nan"), "lr_opt0": 1e-30, "big": 3e38}, 0, 7),
            ({"train_loss_epoch": -1.5}, 0, 300),
            ({"val_rec_loss_epoch": 0.25}, 1, 2 ** 33 + 5)]
    for r in rows:
        w.write(*r)
    w.close()
    d = os.path.join(str(tmp_path), "tensorboard")
    (name,) = os.listdir(d)
    assert name.startswith("events.out.tfevents.") and name.split(".")[3].isdigit()
    version, triples = read_event_file(os.path.join(d, name))
    assert version == "brain.Event:2"
    want = [(k, step, np.float32(v)) for row, _, step in rows for k, v in sorted(row.items())]
    assert len(triples) == len(want)
    for (t, s, v), (wt, ws, wv) in zip(triples, want):
        assert t == wt and s == ws and v.tobytes() == wv.tobytes(), (t, s, v, wt, ws, wv)
    # a second writer in the same second gets a file of its own
    w2 = TensorBoardWriter(str(tmp_path))
    w2.close()
    assert len(os.listdir(d)) == 2


def test_tensorboard_own_loader_agrees(tmp_path):
    loader = pytest.importorskip("tensorboard.backend.event_processing.event_file_loader")
    from dynamicvectorquantization_amd.metrics import TensorBoardWriter
    w = TensorBoardWriter(str(tmp_path))
    w.write({"a_step": 0.5, "b_step": 2.0}, 0, 9)
    w.close()
    d = os.path.join(str(tmp_path), "tensorboard")
    events = list(loader.EventFileLoader(os.path.join(d, os.listdir(d)[0])).Load())
    assert events[0].file_version == "brain.Event:2"
    got = [(v.tag, e.step) for e in events[1:] for v in e.summary.value]
    assert got == [("a_step", 9), ("b_step", 9)]


# ---- CSV -------------------------------------------------------------------------------------------------------------------------------
def _read_csv(path):
    with open(path, newline="") as f:
        r = csv.reader(f)
        header = next(r)
        return header, list(r)


def test_csv_layout_widening_and_resume(tmp_path):
    from dynamicvectorquantization_amd.metrics import CsvWriter, MetricsLogger
    d = str(tmp_path)
    w = CsvWriter(d)
    v = float(np.float32(0.1))
    w.write({"train_loss_step": v, "lr_opt0": 2e-4}, 0, 3)
    w.write({"train_loss_step": 0.25}, 0, 7)
    header, rows = _read_csv(os.path.join(d, "metrics.csv"))
    assert header == ["lr_opt0", "train_loss_step", "epoch", "step"]
    assert rows == [[repr(2e-4), repr(v), "0", "3"], ["", "0.25", "0", "7"]]
    assert np.float32(float(rows[0][1])).tobytes() == np.float32(0.1).tobytes()            # cells round-trip float32 bits
    w.write({"val_rec_loss_epoch": 0.5, "skipped_opt0": 2}, 0, 7)                            # validation keys arrive: the header widens
    header, rows = _read_csv(os.path.join(d, "metrics.csv"))
    assert header == ["lr_opt0", "skipped_opt0", "train_loss_step", "val_rec_loss_epoch", "epoch", "step"]
    assert rows == [[repr(2e-4), "", repr(v), "", "0", "3"], ["", "", "0.25", "", "0", "7"], ["", "2", "", "0.5", "0", "7"]]
    # a second logger on the same directory (a resumed run): earlier rows intact, new rows behind them
    lg = MetricsLogger(d, writers=("csv",), log_every_n_steps=4)
    lg.log_validation({"val_rec_loss": 0.375}, 1, 11)
    lg._write({"train_loss_step": 1.0, "new_key_step": 3.0}, 1, 15)
    lg.close()
    header, rows2 = _read_csv(os.path.join(d, "metrics.csv"))
    assert header == ["lr_opt0", "new_key_step", "skipped_opt0", "train_loss_step", "val_rec_loss_epoch", "epoch", "step"]
    assert [[r[0]] + r[2:] for r in rows2[:3]] == rows and all(r[1] == "" for r in rows2[:3])
    assert rows2[3:] == [["", "", "", "", "0.375", "1", "11"], ["", "3.0", "", "1.0", "", "1", "15"]]
    assert not os.path.exists(os.path.join(d, "metrics.csv.tmp"))


def test_no_logger_means_no_files(tmp_path):
    from dynamicvectorquantization_amd.metrics import MetricsLogger
    lg = MetricsLogger(str(tmp_path), writers=(), log_every_n_steps=4)
    lg.log_validation({"val_rec_loss": 0.375}, 0, 3)
    lg.close()
    assert os.listdir(str(tmp_path)) == []


# ---- the kernels' restatement ------------------------------------------------------------------------------------------------------------
def test_scalar_push_restatement_hand_cases():
    st = TM.new_state(4)
    codes = [TM.F32, TM.I64, TM.IMM, TM.SKIP]
    TM.scalar_push(st, codes, [TM.typed(TM.F32, 0.1), TM.typed(TM.I64, 2 ** 40 + 1), TM.typed(TM.IMM, 0.1), None])
    TM.scalar_push(st, codes, [np.float32("nan"), TM.typed(TM.I64, -3), TM.typed(TM.IMM, float("inf")), None])
    assert st["sum"][0] == np.float64(np.float32(0.1)) and st["cnt"][0] == 1 and st["bad"][0] == 1 and np.isnan(st["last"][0])
    assert st["sum"][1] == float(2 ** 40 - 2) and st["cnt"][1] == 2 and st["last"][1] == np.float32(-3)
    assert st["sum"][2] == 0.1 and st["bad"][2] == 1 and np.isinf(st["last"][2])
    assert st["cnt"][3] == 0 and st["bad"][3] == 0 and st["last"][3] == 0
    assert TM.typed(TM.BF16, 1.00390625) == np.float32(1.0) and TM.typed(TM.BF16, 1.01171875) == np.float32(1.015625)   # ties to even


def test_codebook_health_restatement_hand_cases():
    assert TM.codebook_health(np.zeros(7)) == (0.0, 0.0, 0.0)
    ppl, act, tok = TM.codebook_health([0, 0, 5, 0])
    assert (ppl, act, tok) == (1.0, 1.0, 5.0)
    ppl, act, tok = TM.codebook_health(np.full(1000, 3.0))
    assert abs(ppl - 1000.0) < 1e-9 and act == 1000.0 and tok == 3000.0
    ppl, act, tok = TM.codebook_health([1, 1, 2])
    assert abs(ppl - np.exp(1.5 * np.log(2.0))) < 1e-12 and act == 3.0 and tok == 4.0
