#!/usr/bin/env python3
"""What the device JPEG decode costs and saves (docs/design/23-device-jpeg.md).

Host leg (no GPU needed; --host-only): on a generated file set -- 500 x 375 q90 4:2:0, 500 x 375 q75 4:4:4, 256 x 256 q95 4:2:0,
1024 x 768 q85 4:2:0 -- the time per image, single-threaded and with 16 threads, of
  PIL's full decode to a numpy array, and
  the host pass that is left with device_decode: dvq_jpeg_info + dvq_jpeg_entropy_decode (data.decode_jpeg_host on the file's bytes).
GPU leg: images/s of data.GpuBatchLoader over a generated folder of 500 x 375 q90 4:2:0 files with and without device_decode, in
alternating rounds of one run, and the device stage's time per batch of 64 (HIP events around dvq_jpeg_batch_decode on coefficients
that are already on the device; minimum over rounds).  Writes the table to --out (and prints it).

    python tools/jpeg_timing.py --host-only
    python tools/jpeg_timing.py --out profiles/jpeg_timing.txt
"""
import argparse
import io
import os
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

FILE_SET = [("500x375 q90 4:2:0", 500, 375, dict(quality=90, subsampling=2)), ("500x375 q75 4:4:4", 500, 375, dict(quality=75, subsampling=0)),
            ("256x256 q95 4:2:0", 256, 256, dict(quality=95, subsampling=2)), ("1024x768 q85 4:2:0", 1024, 768, dict(quality=85, subsampling=2))]


def picture(w, h, seed):
    """a photograph-like test picture: smooth shading, a few hard edges, texture and mild sensor noise"""
    import numpy as np
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    ch = []
    for c in range(3):
        a = 120 + 70 * np.sin(xx / (37.0 + 9 * c) + seed) * np.cos(yy / (53.0 - 7 * c)) + 35 * np.sin((xx + 2 * yy) / 11.0 + c)
        a += 40 * ((xx // 61 + yy // 47 + c) % 2) + 12 * np.sin(xx * 0.9) * np.sin(yy * 1.1)
        ch.append(a + rng.normal(0, 4, size=(h, w)))
    return np.clip(np.stack(ch, axis=-1), 0, 255).astype(np.uint8)


def jpeg_bytes(w, h, opts, seed):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(picture(w, h, seed), "RGB").save(buf, "JPEG", **opts)
    return buf.getvalue()


def pil_decode(data):
    import numpy as np
    from PIL import Image
    with Image.open(io.BytesIO(data)) as im:
        return np.asarray(im.convert("RGB") if im.mode != "RGB" else im, dtype=np.uint8)


def per_image_ms(fn, datas, threads, min_seconds):
    """wall time per image of fn over the files, repeated until min_seconds have passed; best of 3"""
    best = float("inf")
    with ThreadPoolExecutor(threads) as pool:
        list(pool.map(fn, datas))
        for _ in range(3):
            n, t0 = 0, time.perf_counter()
            while time.perf_counter() - t0 < min_seconds:
                if threads == 1:
                    for d in datas:
                        fn(d)
                else:
                    list(pool.map(fn, datas * threads))
                n += len(datas) * (1 if threads == 1 else threads)
            best = min(best, (time.perf_counter() - t0) / n)
    return best * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--host-only", action="store_true")
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--seconds", type=float, default=1.0, help="host leg: least duration of a timed window")
    ap.add_argument("--images", type=int, default=1024, help="GPU leg: files in the generated folder")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default="")
    opt = ap.parse_args()
    from dynamicvectorquantization_amd import data as D
    lines = []

    def say(s=""):
        lines.append(s)
        print(s, flush=True)

    say(f"device JPEG decode (tools/jpeg_timing.py); host: {os.cpu_count()} CPUs visible, thread pool of {opt.threads}")
    say("host leg: ms per image, best of 3 windows; PIL = full decode to a numpy array, host pass = dvq_jpeg_info + dvq_jpeg_entropy_decode")
    say(f"  {'file':22s} {'bytes':>8s}  {'PIL x1':>8s} {'pass x1':>8s} {'ratio':>6s}   {'PIL x' + str(opt.threads):>8s} {'pass x' + str(opt.threads):>8s} {'ratio':>6s}")
    tot = [0.0, 0.0]
    for label, w, h, o in FILE_SET:
        datas = [jpeg_bytes(w, h, o, s) for s in range(4)]
        assert all(D.decode_jpeg_host(d) is not None for d in datas)
        row = []
        for threads in (1, opt.threads):
            a = per_image_ms(pil_decode, datas, threads, opt.seconds)
            b = per_image_ms(D.decode_jpeg_host, datas, threads, opt.seconds)
            row += [a, b, b / a]
        tot[0] += row[0]
        tot[1] += row[1]
        say(f"  {label:22s} {sum(map(len, datas)) // 4:8d}  {row[0]:8.3f} {row[1]:8.3f} {row[2]:6.3f}   {row[3]:8.3f} {row[4]:8.3f} {row[5]:6.3f}")
    say(f"  single-threaded, the four kinds summed: PIL {tot[0]:.3f} ms, host pass {tot[1]:.3f} ms, ratio {tot[1] / tot[0]:.3f}")
    if not opt.host_only:
        gpu_leg(opt, say)
    if opt.out:
        os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
        with open(opt.out, "w") as f:
            f.write("\n".join(lines) + "\n")


def gpu_leg(opt, say):
    import torch
    assert torch.cuda.is_available(), "the GPU leg needs an MI355X (--host-only for the host leg alone)"
    dev = torch.device("cuda:0")
    from dynamicvectorquantization_amd import kernels as K
    tf, mhz = K.probe_mfma_rate(True)          # the box's sustained clock, as bench.py reports it (docs/design/07-measurement.md)
    clock = f"matrix pipes sustain {tf:.0f} TFLOP/s at {mhz:.0f} MHz"
    say()
    say(f"GPU leg: {torch.cuda.get_device_name(0)}, {clock}")
    with tempfile.TemporaryDirectory(prefix="dvq_jpeg_timing_") as root:
        gpu_leg_in(root, opt, say, dev)


def gpu_leg_in(root, opt, say, dev):
    import torch

    from dynamicvectorquantization_amd import data as D
    from dynamicvectorquantization_amd.kernels import _p, _s, check, lib
    os.makedirs(os.path.join(root, "c0"))
    label, w, h, o = FILE_SET[0]
    distinct = [jpeg_bytes(w, h, o, s) for s in range(16)]
    for i in range(opt.images):
        with open(os.path.join(root, "c0", f"{i:06d}.jpg"), "wb") as f:
            f.write(distinct[i % 16])

    def rate(device_decode):
        loader = D.GpuBatchLoader(D.ImageFolder(root), opt.batch, dev, size=256, num_workers=opt.threads, device_decode=device_decode)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        n = 0
        for b in loader:
            n += int(b["image"].shape[0])
        torch.cuda.synchronize()
        return n / (time.perf_counter() - t0)
    rate(False), rate(True)                       # warm: file cache, code objects, pinned pools
    res = {False: [], True: []}
    for _ in range(opt.rounds):
        for dd in (False, True):
            res[dd].append(rate(dd))
    say(f"  GpuBatchLoader over {opt.images} files ({label}), batch {opt.batch}, {opt.threads} host threads, eval transform to 256 x 256; "
        f"{opt.rounds} alternating rounds, images/s:")
    for dd in (False, True):
        say(f"    device_decode={str(dd):5s}  " + "  ".join(f"{v:9.1f}" for v in res[dd]) + f"   max {max(res[dd]):9.1f}")
    say(f"    on / off: {max(res[True]) / max(res[False]):.3f}")

    recs = [D.decode_jpeg_host(distinct[i % 16]) for i in range(opt.batch)]
    D.decode_batch_gpu(recs, dev)                 # warm
    # the same launch pair on buffers that are already resident: what the device stage itself takes
    import numpy as np
    descs, coef_len, plane_len, rgb_len, _, _ = D.jpeg_batch_layout(recs)
    coef = torch.from_numpy(np.concatenate([r["coef"] for r in recs])).to(dev)
    desc = torch.from_numpy(np.frombuffer(bytes(descs), dtype=np.uint8).copy()).to(dev)
    planes = torch.empty(plane_len, dtype=torch.uint8, device=dev)
    rgb = torch.empty(rgb_len, dtype=torch.uint8, device=dev)

    def stage():
        check(lib().dvq_jpeg_batch_decode(_p(coef), _p(desc), opt.batch, _p(planes), _p(rgb), _s()), "dvq_jpeg_batch_decode")
    for _ in range(5):
        stage()
    best = float("inf")
    for _ in range(opt.rounds):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        torch.cuda.synchronize()
        ev[0].record()
        for _ in range(20):
            stage()
        ev[1].record()
        torch.cuda.synchronize()
        best = min(best, ev[0].elapsed_time(ev[1]) / 20)
    moved = coef_len * 2 + 2 * plane_len + rgb_len
    say(f"  device stage (dvq_jpeg_batch_decode: IDCT + upsample / colour), batch of {opt.batch} {label}: {best:.4f} ms per batch, "
        f"min of {opt.rounds} x 20 calls = {opt.batch / best * 1e3:.0f} images/s; {moved / 1e6:.1f} MB read and written "
        f"-> {moved / best / 1e6:.1f} GB/s")


if __name__ == "__main__":
    main()
