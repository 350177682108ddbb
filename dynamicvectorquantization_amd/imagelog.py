"""Training-time image logging (docs/design/18-image-logging.md).

* the reference's grain pictures (modules/dynamic_modules/utils.py:41-161) under their own names and arguments, on device tensors:
  draw_dual_grain_256res_color / draw_triple_grain_256res_color (colour overlays, kernels.grain_overlay) and draw_dual_grain_256res /
  draw_triple_grain_256res (grid lines, kernels.grain_lines_).  The cell size is H // h where the reference hard-codes 256 // h.
* ImageLogger: utils/logger.py:57-147 (CaptionImageLogger.log_img + log_local) without Lightning.  Every `batch_frequency` batches
  the model's `log_images` runs in eval mode under no_grad; each panel's first `max_images` images become ONE 8-bit grid on the device
  (kernels.image_grid_u8, on a side stream), the grid is copied asynchronously into pinned memory, and a single writer thread encodes
  the PNG once the copy's event has completed.  The training loop pays for the eval forward and a few launches; only bytes cross to the
  host.  There is no host fallback: a panel that is not a device tensor raises.
"""
from __future__ import annotations

import atexit
import os
import queue
import threading

import torch

from . import kernels as K

color_dict = {
    "red": (255, 0, 0),
    "green": (0, 255, 0),
    "white": (255, 255, 255),
    "yellow": (255, 255, 0),
    "blue": (5, 39, 175),
}


def _images_for(images, indices, name):
    if indices is None:
        raise ValueError(f"{name}: `indices` ([batch, height, width]) is required")
    if images is None:                          # the reference: torch.ones(B, 3, 256, 256)
        images = torch.ones(indices.size(0), 3, 256, 256, dtype=torch.float32, device=indices.device)
    if images.dtype != torch.float32 or not images.is_contiguous():
        images = images.float().contiguous()
    return images


def _overlay(images, indices, levels, low_color, high_color, scaler, name):
    images = _images_for(images, indices, name)
    low, high = color_dict[low_color], color_dict[high_color]
    if indices.is_floating_point():             # a score map in [0, 1] (the entropy picture); the triple form halves it like the reference
        score = indices.float().contiguous() if levels == 2 else (indices.float() / 2).contiguous()
        return K.grain_overlay(images, score=score, low=low, high=high, scaler=scaler)
    return K.grain_overlay(images, grain=indices.long().contiguous(), levels=levels, low=low, high=high, scaler=scaler)


def draw_dual_grain_256res_color(images=None, indices=None, low_color="blue", high_color="red", scaler=0.9):
    """indices [B,h,w]: 0 coarse / 1 fine (int), or a float score map -> the range-normalised images blended towards low / high colour"""
    return _overlay(images, indices, 2, low_color, high_color, scaler, "draw_dual_grain_256res_color")


def draw_triple_grain_256res_color(images=None, indices=None, low_color="blue", high_color="red", scaler=0.9):
    """indices [B,h,w]: 0 coarse / 1 median / 2 fine"""
    return _overlay(images, indices, 3, low_color, high_color, scaler, "draw_triple_grain_256res_color")


def _lines(images, indices, levels, name):
    given = images
    images = _images_for(images, indices, name)
    K.grain_lines_(images, indices.long().contiguous(), levels)
    if given is not None and given is not images:           # the reference draws into its argument
        given.copy_(images)
        return given
    return images


def draw_dual_grain_256res(images=None, indices=None):
    """-1 on every cell's top row and left column, and on the middle row and column of fine cells; in place, returns `images`"""
    return _lines(images, indices, 2, "draw_dual_grain_256res")


def draw_triple_grain_256res(images=None, indices=None):
    """as the dual form, plus the quarter lines of grain-2 cells"""
    return _lines(images, indices, 3, "draw_triple_grain_256res")


def normalize_scores(x):
    """dqvae_dual_entropy.py:254: x.sub(x.min()).div(max(x.max() - x.min(), 1e-5)) -- over the whole batch, without a host read"""
    lo, hi = torch.aminmax(x)
    return x.sub(lo).div(torch.clamp_min(hi - lo, 1e-5))


# ---------------------------------------------------------------------------------------------
class _Event:
    __slots__ = ("done", "grids", "keep")

    def __init__(self, done, grids, keep):
        self.done, self.grids, self.keep = done, grids, keep


class ImageLogger:
    """`maybe_log(model, batch, batch_idx, split)` after a train step / a validation batch; `flush()` before the files are read and
    before the process ends (Trainer.fit does, and an atexit hook).  Rank 0 only.  At most `QUEUE` log events wait for the writer: a
    third one blocks the caller until a slot frees, instead of pinning more memory."""

    QUEUE = 2
    PADDING = 2

    def __init__(self, save_dir, batch_frequency=50, max_images=16, clamp=True, nrow=4, seed=2021):
        self.save_dir, self.batch_freq, self.max_images = save_dir, int(batch_frequency), int(max_images)
        self.clamp, self.nrow, self.seed = bool(clamp), int(nrow), int(seed)
        self.written = []                       # paths, in writing order
        self.events = 0
        self._q = None
        self._thread = None
        self._error = None
        self._stream = None
        self._sampler_state = None              # device {seed, counter} of the stage-2 sampling draws: the logger's own stream
        atexit.register(self.flush)

    # ---- which batches ----------------------------------------------------------------------------------------------------------
    @staticmethod
    def _rank0():
        import torch.distributed as dist
        return not (dist.is_available() and dist.is_initialized()) or dist.get_rank() == 0

    def due(self, model, batch_idx):
        return (self.batch_freq > 0 and self.max_images > 0 and batch_idx % self.batch_freq == 0 and
                callable(getattr(model, "log_images", None)) and self._rank0())

    def sampler_state(self, device):
        st = self._sampler_state
        if st is None or st.device != torch.device(device):
            st = self._sampler_state = torch.tensor([self.seed & 0x7FFFFFFFFFFFFFFF, 0], dtype=torch.int64, device=device)
        return st

    # ---- one event --------------------------------------------------------------------------------------------------------------
    def maybe_log(self, model, batch, batch_idx, split="train"):
        """-> True if this batch was logged"""
        if not self.due(model, batch_idx):
            return False
        self._raise_pending()
        flags = [(m, m.training) for m in model.modules()]
        model.eval()
        try:
            with torch.no_grad():
                dev = next(model.parameters()).device
                images = model.log_images(batch, split=split, max_images=self.max_images, sampler_state=self.sampler_state(dev))
        finally:
            for m, was in flags:                # every submodule as found (a frozen first stage stays in eval mode)
                m.training = was
        self.log_local(split, images, int(getattr(model, "global_step", 0)), int(getattr(model, "current_epoch", 0)), batch_idx)
        return True

    def log_local(self, split, images, global_step, current_epoch, batch_idx):
        """utils/logger.py:122-147: first max_images of every panel, clamp, make_grid(nrow, normalize=True), * 255 -> PNG"""
        panels = {}
        for k, v in images.items():
            if not torch.is_tensor(v):
                continue                        # captions of the text models: not pictures
            if not v.is_cuda:
                raise TypeError(f"log_images['{k}'] is a CPU tensor: panels are made on the device")
            v = v[:min(v.shape[0], self.max_images)].detach()
            panels[k] = v if v.dtype == torch.float32 and v.is_contiguous() else v.float().contiguous()
        if not panels:
            return
        dev = next(iter(panels.values())).device
        root = os.path.join(self.save_dir, "images", split)
        if self._stream is None or self._stream.device != dev:
            self._stream = torch.cuda.Stream(device=dev)
        side = self._stream
        side.wait_stream(torch.cuda.current_stream(dev))
        grids, keep = [], []
        with torch.cuda.stream(side):
            ws = K.imagelog_workspace(1, dev)
            for k, v in panels.items():
                g = K.image_grid_u8(v, nrow=self.nrow, padding=self.PADDING, clamp=self.clamp, ws=ws)
                host = torch.empty(g.shape, dtype=torch.uint8, pin_memory=True)
                host.copy_(g, non_blocking=True)
                name = "Step_{:06}-Epoch_{:03}-Batch_{:06}-{}.png".format(global_step, current_epoch, batch_idx, k)
                grids.append((os.path.join(root, name), host))
                keep += [v, g]                  # alive until the copies have run: these were not allocated on the side stream
            keep.append(ws)
            done = torch.cuda.Event()
            done.record(side)
        self.events += 1
        self._writer().put(_Event(done, grids, keep))         # blocks while QUEUE events are waiting

    # ---- the writer -------------------------------------------------------------------------------------------------------------
    def _writer(self):
        if self._thread is None or not self._thread.is_alive():
            self._q = queue.Queue(maxsize=self.QUEUE)
            self._thread = threading.Thread(target=self._run, args=(self._q,), name="dvq-image-writer", daemon=True)
            self._thread.start()
        return self._q

    def _run(self, q):
        from PIL import Image
        while True:
            ev = q.get()
            if ev is None:
                return
            try:
                if self._error is None:
                    ev.done.synchronize()
                    ev.keep = None
                    for path, host in ev.grids:
                        os.makedirs(os.path.dirname(path), exist_ok=True)
                        Image.fromarray(host.numpy()).save(path)
                        self.written.append(path)
            except BaseException as e:          # reported by the next maybe_log / flush on the caller's thread
                self._error = e

    def _raise_pending(self):
        if self._error is not None:
            e, self._error = self._error, None
            raise RuntimeError("the image writer failed") from e

    def flush(self):
        """every queued picture is on disk when this returns (the writer thread is joined; the next event starts a new one)"""
        t = self._thread
        if t is not None and t.is_alive():
            self._q.put(None)
            t.join()
        self._thread = None
        self._raise_pending()
