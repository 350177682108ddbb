#!/usr/bin/env python3
"""Generate tests/golden/imagelog.npz by running the REAL reference draw functions (modules/dynamic_modules/utils.py:41-161) on the CPU
(build container only).  Not imported by tests, bench.py or __graft_entry__.py.

    python tools/gen_golden_imagelog.py /path/to/reference

The inputs come from tests/imagelog_cpu.py (seeded, shared with the tests); the fixture holds the reference's OUTPUTS as bytes.  PIL's
Image.blend, numpy's casts and the reference's own draw code are the real thing.  torchvision is not installed where this runs, so three
of its functions are restated HERE, in-process, for the reference to import (container-only, as gen_golden.py does for
pytorch_lightning):
    ToPILImage            pic.mul(255).byte(), CHW -> HWC
    functional.to_tensor  HWC uint8 -> CHW, .div(255)
    utils.make_grid       the 4-D branch: one channel repeated to three, normalize over the whole tensor with the 1e-5 floor, a single
                          image returned as it is, else images laid out nrow per row with `padding` zeros around each
The `grid*` entries therefore pin this file's restatement of make_grid followed by utils/logger.py:140-143's `(grid * 255).astype(uint8)`
-- not torchvision itself.  While writing, every entry is compared with tests/imagelog_cpu.py's restatement: a mismatch stops the run.
"""
from __future__ import annotations

import math
import os
import sys
import types

import numpy as np
import torch
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(REPO, "tests"))

import imagelog_cpu as IC  # noqa: E402


def make_grid(tensor, nrow=8, padding=2, normalize=False, pad_value=0.0):
    assert tensor.dim() == 4
    if tensor.size(1) == 1:
        tensor = torch.cat((tensor, tensor, tensor), 1)
    if normalize:
        tensor = tensor.clone()
        low, high = float(tensor.min()), float(tensor.max())
        tensor.clamp_(min=low, max=high)
        tensor.sub_(low).div_(max(high - low, 1e-5))
    if tensor.size(0) == 1:
        return tensor.squeeze(0)
    nmaps = tensor.size(0)
    xmaps = min(nrow, nmaps)
    ymaps = int(math.ceil(float(nmaps) / xmaps))
    height, width = int(tensor.size(2) + padding), int(tensor.size(3) + padding)
    grid = tensor.new_full((tensor.size(1), height * ymaps + padding, width * xmaps + padding), pad_value)
    k = 0
    for y in range(ymaps):
        for x in range(xmaps):
            if k >= nmaps:
                break
            grid.narrow(1, y * height + padding, height - padding).narrow(2, x * width + padding, width - padding).copy_(tensor[k])
            k += 1
    return grid


def install_stubs():
    tv = types.ModuleType("torchvision")
    tvt = types.ModuleType("torchvision.transforms")
    tvf = types.ModuleType("torchvision.transforms.functional")
    tvu = types.ModuleType("torchvision.utils")

    class ToPILImage:
        def __call__(self, pic):
            return Image.fromarray(np.transpose(pic.mul(255).byte().numpy(), (1, 2, 0)), mode="RGB")

    class Compose:
        def __init__(self, ts):
            self.ts = ts

        def __call__(self, x):
            for f in self.ts:
                x = f(x)
            return x

    def to_tensor(pic):
        a = torch.from_numpy(np.array(pic, dtype=np.uint8, copy=True))
        return a.permute(2, 0, 1).contiguous().to(torch.float32).div(255)

    tvt.ToPILImage, tvt.Compose, tvt.functional = ToPILImage, Compose, tvf
    tvf.to_tensor = to_tensor
    tvu.make_grid = make_grid
    tv.transforms, tv.utils = tvt, tvu
    sys.modules.update({"torchvision": tv, "torchvision.transforms": tvt, "torchvision.transforms.functional": tvf,
                        "torchvision.utils": tvu})


def as_bytes(t):
    """fp32 k / 255 -> k (exact: checked)"""
    a = t.numpy()
    k = np.rint(a * 255.0).astype(np.uint8)
    assert np.array_equal(k.astype(np.float32) / np.float32(255), a), "a colour panel is not k / 255"
    return k


def same(name, ref, mine):
    if not np.array_equal(ref, mine):
        raise SystemExit(f"{name}: tests/imagelog_cpu.py differs from the reference on {int((ref != mine).sum())} of {ref.size} values")
    print(f"  {name}: {ref.shape} matches the restatement")


def main():
    if len(sys.argv) != 2 or not os.path.isdir(sys.argv[1]):
        raise SystemExit(__doc__)
    install_stubs()
    sys.path.insert(0, os.path.abspath(sys.argv[1]))
    from modules.dynamic_modules import utils as U

    B = IC.FIXTURE_BATCH
    x = IC.fixture_images()
    g2, g3, sc = IC.fixture_grain(B, 16, 16, 2), IC.fixture_grain(B, 8, 8, 3), IC.fixture_score(B, 16, 16)
    t = torch.from_numpy
    out = {"seed": np.int64(IC.FIXTURE_SEED)}

    out["dual_color"] = as_bytes(U.draw_dual_grain_256res_color(images=t(x).clone(), indices=t(g2), scaler=0.7))
    same("dual_color", out["dual_color"], as_bytes(t(IC.overlay(x, grain=g2, levels=2, scaler=0.7))))
    out["triple_color"] = as_bytes(U.draw_triple_grain_256res_color(images=t(x).clone(), indices=t(g3)))
    same("triple_color", out["triple_color"], as_bytes(t(IC.overlay(x, grain=g3, levels=3, scaler=0.9))))
    out["score_color"] = as_bytes(U.draw_dual_grain_256res_color(images=t(x).clone(), indices=t(sc), scaler=0.7))
    same("score_color", out["score_color"], as_bytes(t(IC.overlay(x, score=sc, scaler=0.7))))
    # images=None: ones with -1 on the lines -> stored as the line mask
    for name, fn, g, lv in (("dual_lines", U.draw_dual_grain_256res, g2, 2), ("triple_lines", U.draw_triple_grain_256res, g3, 3)):
        r = fn(indices=t(g)).numpy()
        assert np.isin(r, (1.0, -1.0)).all() and (r[:, :1] == r).all()
        out[name] = (r[:, 0] == -1.0).astype(np.uint8)
        same(name, out[name], IC.line_mask(g, 256, 256).astype(np.uint8))
        # on a real image: untouched pixels keep their value
        r2 = fn(images=t(x).clone(), indices=t(g)).numpy()
        same(name + " (on images)", r2, IC.lines(x, g, lv))
    # utils/logger.py:122-143 on small panels: clamp, make_grid(nrow=4, normalize=True), HWC, (grid * 255).astype(uint8)
    rng = np.random.default_rng(IC.FIXTURE_SEED + 5)
    for name, shape in (("grid5", (5, 3, 20, 12)), ("grid1", (1, 3, 9, 7)), ("grid4_c1", (4, 1, 6, 10))):
        v = (rng.integers(-300, 301, size=shape).astype(np.float32) / np.float32(200)).astype(np.float32)      # some outside [-1, 1]
        out[name + "_in"] = v
        for clamp in (True, False):
            tv = torch.clamp(t(v), -1., 1.) if clamp else t(v)
            grid = make_grid(tv, nrow=4, normalize=True)
            grid = grid.transpose(0, 1).transpose(1, 2).squeeze(-1).numpy()
            key = f"{name}_{'clamp' if clamp else 'raw'}"
            out[key] = (grid * 255).astype(np.uint8)
            same(key, out[key], IC.grid_u8(v, nrow=4, padding=2, clamp=clamp))
    path = os.path.join(REPO, "tests", "golden", "imagelog.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
