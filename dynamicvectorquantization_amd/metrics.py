"""Training metric logs (docs/design/22-metrics-logging.md): what the reference gets from `self.log(..., on_step=True, on_epoch=True)`
through Lightning's loggers (train.py:125-150) -- every scalar a model hands to its `log` / `log_dict` shim as `<name>_step` every
`log_every_n_steps` steps and as `<name>_epoch` (the mean over the epoch) at epoch ends -- written as `metrics.csv` in the layout of
Lightning's CSVLogger and / or as a TensorBoard event file, with no dependency beyond the standard library.

The step stays free of host reads: one `dvq_scalar_push` at the end of the (recorded) step gathers the step's scalars into a device
state block -- last value, fp64 running sum, counts -- and the host copies that block once per row.  The EMA quantiser's per-code
counts of the step go through `dvq_codebook_health` into three more columns (perplexity, active codes, tokens).

    lg = MetricsLogger(logdir, writers=("csv", "tensorboard"), log_every_n_steps=50)
    Trainer(model, ..., metrics_logger=lg).fit(...)

Rank 0 writes its own values (Lightning's behaviour for keys logged without sync_dist); nothing is averaged over ranks.
"""
from __future__ import annotations

import csv
import os
import socket
import struct
import time

WRITERS = ("csv", "tensorboard")


def parse_logger_flag(spec):
    """`-l/--logger` of train.py: none | csv | tensorboard | a comma list -> (writers, names accepted and ignored).  `wandb` (the
    reference's other choice) is accepted and ignored; anything else raises ValueError"""
    names = [s.strip().lower() for s in str(spec or "none").split(",") if s.strip()]
    writers, ignored = [], []
    for n in names:
        if n in WRITERS:
            if n not in writers:
                writers.append(n)
        elif n == "wandb":
            ignored.append(n)
        elif n not in ("none", "false", "off"):
            raise ValueError(f"--logger {spec!r}: unknown logger {n!r} (none, csv, tensorboard or a comma list of these)")
    return tuple(writers), ignored


# ---- CRC-32C (Castagnoli), table-driven ----------------------------------------------------------------------------------------------
def _crc32c_table():
    table = []
    for i in range(256):
        c = i
        for _ in range(8):
            c = (c >> 1) ^ 0x82F63B78 if c & 1 else c >> 1
        table.append(c)
    return tuple(table)


_CRC_TABLE = _crc32c_table()


def crc32c(data: bytes) -> int:
    c = 0xFFFFFFFF
    for b in data:
        c = _CRC_TABLE[(c ^ b) & 0xFF] ^ (c >> 8)
    return c ^ 0xFFFFFFFF


def masked_crc32c(data: bytes) -> int:
    """the checksum as TFRecord files store it"""
    c = crc32c(data)
    return ((c >> 15 | c << 17) + 0xA282EAD8) & 0xFFFFFFFF


# ---- protobuf, by hand: the four fields of Event and the two of Summary.Value that scalars need --------------------------------------
def _varint(n: int) -> bytes:
    n &= 0xFFFFFFFFFFFFFFFF
    out = bytearray()
    while n >= 0x80:
        out.append((n & 0x7F) | 0x80)
        n >>= 7
    out.append(n)
    return bytes(out)


def _bytes_field(number: int, payload: bytes) -> bytes:
    return _varint(number << 3 | 2) + _varint(len(payload)) + payload


def encode_event(wall_time, step=0, file_version=None, scalars=None) -> bytes:
    """tensorflow.Event: wall_time (1, double), step (2, int64), file_version (3, string) or summary (5) holding one
    Summary.Value {tag (1, string), simple_value (2, float)} per scalar"""
    ev = b"\x09" + struct.pack("<d", float(wall_time))
    if step:
        ev += b"\x10" + _varint(int(step))
    if file_version is not None:
        ev += _bytes_field(3, file_version.encode("utf-8"))
    if scalars is not None:
        summary = b"".join(_bytes_field(1, _bytes_field(1, tag.encode("utf-8")) + b"\x15" + struct.pack("<f", float(v)))
                           for tag, v in scalars)
        ev += _bytes_field(5, summary)
    return ev


def tfrecord(payload: bytes) -> bytes:
    """length, masked CRC-32C of the length, payload, masked CRC-32C of the payload"""
    head = struct.pack("<Q", len(payload))
    return head + struct.pack("<I", masked_crc32c(head)) + payload + struct.pack("<I", masked_crc32c(payload))


class TensorBoardWriter:
    """<logdir>/tensorboard/events.out.tfevents.<secs>.<host>: one Event per row, every key of the row a scalar of its Summary.  A
    resumed run adds a second file to the directory, which TensorBoard reads as one run."""

    def __init__(self, logdir):
        d = os.path.join(logdir, "tensorboard")
        os.makedirs(d, exist_ok=True)
        base = os.path.join(d, f"events.out.tfevents.{int(time.time())}.{socket.gethostname()}")
        self.path, n = base, 0
        while os.path.exists(self.path):          # two writers within one second
            n += 1
            self.path = f"{base}.{n}"
        self._f = open(self.path, "wb")
        self._f.write(tfrecord(encode_event(time.time(), file_version="brain.Event:2")))
        self._f.flush()

    def write(self, row, epoch, step):
        if not row:
            return
        if self._f.closed:                        # a second fit() with the same logger
            self._f = open(self.path, "ab")
        self._f.write(tfrecord(encode_event(time.time(), step=step, scalars=sorted(row.items()))))
        self._f.flush()

    def close(self):
        if not self._f.closed:
            self._f.close()


class CsvWriter:
    """<logdir>/metrics.csv as Lightning's CSVLogger lays it out: one row per event, the sorted union of the keys, then `epoch` and
    `step`; cells of absent keys are empty.  A key not seen before widens the header: the file is rewritten (through a temporary file)
    with the earlier rows intact.  An existing file -- a resumed run -- is continued."""
    TAIL = ("epoch", "step")

    def __init__(self, logdir):
        os.makedirs(logdir, exist_ok=True)
        self.path = os.path.join(logdir, "metrics.csv")
        self.keys = []
        if os.path.exists(self.path):
            with open(self.path, newline="") as f:
                header = next(csv.reader(f), [])
            self.keys = [k for k in header if k not in self.TAIL]

    @staticmethod
    def _cell(v):
        return v if isinstance(v, str) else repr(int(v)) if isinstance(v, int) else repr(float(v))

    def _widen(self, keys):
        rows = []
        if os.path.exists(self.path):
            with open(self.path, newline="") as f:
                rows = list(csv.DictReader(f))
        self.keys = sorted(set(self.keys) | set(keys))
        tmp = self.path + ".tmp"
        with open(tmp, "w", newline="") as f:
            w = csv.DictWriter(f, fieldnames=self.keys + list(self.TAIL), restval="")
            w.writeheader()
            w.writerows(rows)
        os.replace(tmp, self.path)

    def write(self, row, epoch, step):
        if not row:
            return
        if not set(row) <= set(self.keys) or not os.path.exists(self.path):
            self._widen(row)
        with open(self.path, "a", newline="") as f:
            w = csv.DictWriter(f, fieldnames=self.keys + list(self.TAIL), restval="")
            w.writerow({**{k: self._cell(v) for k, v in row.items()}, "epoch": int(epoch), "step": int(step)})

    def close(self):
        pass


# ---- the logger ----------------------------------------------------------------------------------------------------------------------
CODEBOOK_KEYS = ("train_codebook_perplexity", "train_codebook_active", "train_codebook_tokens")


def codebook_counts(model):
    """(counts view, K, element stride) of the per-code counts the model's EMA quantiser left on the device in its last training
    forward -- column D of VQEmbedding's persistent [K, D + 1] statistics buffer, global counts after the data-parallel exchange,
    left intact by vq_ema_apply -- or None: no such quantiser (stage 2, MaskVectorQuantize), or no training forward yet"""
    cb = getattr(getattr(model, "quantize", None), "codebook", None)
    xb = getattr(cb, "_xchg", None)
    if xb is None or not getattr(cb, "ema", False):
        return None
    stats = xb[1]
    k, d1 = stats.shape
    return stats[:, d1 - 1], int(k), int(d1)


class MetricsLogger:
    """Scalar logs of a training run.  `writers`: names out of WRITERS; `log_every_n_steps`: Lightning's flag of the same name (a `_step` row after every n-th step).  The Trainer drives it: attach() once,
    push() inside every step, after_step() behind it, log_validation() and finish() from fit."""
    COLUMNS = 256

    def __init__(self, logdir, writers=("csv",), log_every_n_steps=50):
        self.logdir = logdir
        self.log_every_n_steps = max(1, int(log_every_n_steps))
        self.writers = [{"csv": CsvWriter, "tensorboard": TensorBoardWriter}[w](logdir) for w in writers]
        self.columns = {}                  # key -> column of the state block, in order of first sight
        self.state = None
        self.rows_written = 0
        self.last_keys = ()                # keys the last step pushed (a replayed step: those of its recording, set by the Trainer)
        self._health = self._cb_total = None
        self._t_row, self._images = None, 0

    # -- device side ---------------------------------------------------------------------------------------------------------------
    def attach(self, model, device):
        """allocate the state block (and the quantiser's running total) -- before any step, never inside one: a recorded step holds
        their addresses"""
        import torch
        from . import kernels as K
        self.state = K.scalar_push_state(self.COLUMNS, device)
        self._health = torch.zeros(3, dtype=torch.float32, device=device)
        cb = getattr(getattr(model, "quantize", None), "codebook", None)
        if getattr(cb, "ema", False) and hasattr(cb, "n_embed"):
            self._cb_total = torch.zeros(int(cb.n_embed), dtype=torch.float64, device=device)

    def _column(self, key):
        c = self.columns.get(key)
        if c is None:
            if len(self.columns) >= self.COLUMNS:
                raise RuntimeError(f"metrics logger: more than {self.COLUMNS} distinct keys (at {key!r})")
            c = self.columns[key] = len(self.columns)
        return c

    def push(self, model, logged):
        """the step's launches: dvq_codebook_health when the model has an EMA quantiser, then one dvq_scalar_push per 64 columns.
        `logged`: what the model's log shim collected in THIS step; a key missing from it keeps its column untouched."""
        import torch
        from . import kernels as K
        values = {}
        for k, v in logged.items():
            if torch.is_tensor(v):
                if v.numel() != 1:
                    continue
                values[k] = v if v.is_cuda else float(v)          # a host tensor (the loss's disc_factor) is a host number
            elif isinstance(v, (int, float)):
                values[k] = float(v)
        cc = codebook_counts(model) if self._cb_total is not None and model.training else None
        if cc is not None:
            counts, k, stride = cc
            K.codebook_health(counts, k, stride, self._health, total=self._cb_total)
            for i, key in enumerate(CODEBOOK_KEYS):
                values[key] = self._health[i:i + 1]
        self.last_keys = tuple(values)
        if not values:
            return
        for k in values:
            self._column(k)
        slots = [None] * len(self.columns)
        for k, v in values.items():
            slots[self.columns[k]] = v
        K.scalar_push(slots, self.state, self.COLUMNS)

    # -- host side -----------------------------------------------------------------------------------------------------------------
    def _write(self, row, epoch, step):
        for w in self.writers:
            w.write(row, epoch, step)
        self.rows_written += 1

    def _read_state(self):
        from . import kernels as K
        return K.scalar_push_views(self.state.cpu(), self.COLUMNS)          # ONE device-to-host copy

    def after_step(self, trainer, step, batch=None, lrs=None):
        """`step`: index of the step just taken.  Writes the `_step` row when (step + 1) is a multiple of log_every_n_steps and the
        `_epoch` row when it is a multiple of the model's steps_per_epoch"""
        import torch
        spe = max(1, int(getattr(trainer.model, "steps_per_epoch", 1) or 1))
        if batch is not None:
            self._images += next((int(v.shape[0]) for v in batch.values() if torch.is_tensor(v) and v.dim() > 0), 0)
        if self._t_row is None:
            self._t_row, self._images = time.perf_counter(), 0          # the rate counts from the end of the first step seen
        if (step + 1) % self.log_every_n_steps == 0 and self.last_keys:
            _, _, _, last = self._read_state()                             # synchronises: the step has finished
            row = {f"{k}_step": float(last[self.columns[k]]) for k in self.last_keys}
            for i, lr in enumerate(lrs or []):
                row[f"lr_opt{i}"] = float(lr)
            now = time.perf_counter()
            if self._images and now > self._t_row:
                row["images_per_sec"] = self._images / (now - self._t_row)
            self._t_row, self._images = now, 0
            if trainer.grad_guard_enabled:
                for i, st in enumerate(trainer.grad_stats()):
                    if st:
                        row.update({f"grad_norm_opt{i}": st["norm"], f"clip_coef_opt{i}": st["coef"], f"skipped_opt{i}": st["skipped"]})
            nt = getattr(trainer, "norm_tracker", None)          # per-parameter norm tracking: the totals its row of THIS step left
            if nt is not None and nt.last_row[0] == step:
                row.update(nt.last_row[1])
            self._write(row, step // spe, step)
        if (step + 1) % spe == 0:
            self.epoch_end(step // spe, step)

    def epoch_end(self, epoch, step):
        """`<key>_epoch` = sum / cnt of the finite values pushed since the last call, the codebook figures of the epoch's usage; then the
        sums restart"""
        import torch
        if self.state is None or not self.columns:
            return
        s, cnt, bad, _ = self._read_state()
        row = {f"{k}_epoch": float(s[c]) / int(cnt[c]) for k, c in self.columns.items() if int(cnt[c]) > 0}
        nbad = int(bad.sum())
        if nbad:
            row["nonfinite_values_epoch"] = nbad
        if self._cb_total is not None and f"{CODEBOOK_KEYS[0]}_epoch" in row:
            # usage of the whole epoch, not the mean of the steps' figures: a code counts as dead only if no step used it
            tot = self._cb_total.cpu()
            n = float(tot.sum())
            if n > 0:
                p = tot[tot > 0] / n
                row[f"{CODEBOOK_KEYS[0]}_epoch"] = float(torch.exp(-(p * torch.log(p)).sum()))
                row["train_codebook_dead_epoch"] = int((tot == 0).sum())
            self._cb_total.zero_()
        if row:
            self._write(row, epoch, step)
        self.state.zero_()                    # a launch of its own, outside any recording

    def log_validation(self, metrics, epoch, step):
        """the averaged dict of Trainer.validate as `<key>_epoch`"""
        if metrics:
            self._write({f"{k}_epoch": float(v) for k, v in metrics.items()}, epoch, step)

    def finish(self, trainer):
        """end of fit: the epoch row of a partial epoch, files closed"""
        step = int(trainer.model.global_step) - 1
        spe = max(1, int(getattr(trainer.model, "steps_per_epoch", 1) or 1))
        if step >= 0 and (step + 1) % spe != 0:
            self.epoch_end(step // spe, step)
        self.close()

    def close(self):
        for w in self.writers:
            w.close()
