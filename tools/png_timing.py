#!/usr/bin/env python3
"""What the device PNG decode costs and saves (docs/design/29-device-png.md).

Host leg (no GPU needed; --host-only): on generated photograph-like RGB files of 256 x 256 and 1024 x 1024 (PIL's encoder, which picks a
filter per row) the time per image, single-threaded and with 16 threads, of
  PIL's full decode to a numpy array,
  the host pass that is left with device_png: chunk walk, CRCs, bounded inflate, length and filter-byte checks (data.decode_png_host), and
  zlib's inflate of the IDAT stream alone.
GPU leg: images/s of data.GpuBatchLoader over generated folders with device_png off (the baseline: PIL) and on, in alternating rounds of
one run, and the device stage's time per batch of 64 at 1024 x 1024 (HIP events around dvq_png_batch_unfilter on scanlines that are
already on the device; minimum over rounds).  Writes the table to --out (and prints it).

    python tools/png_timing.py --host-only
    python tools/png_timing.py --out profiles/png_timing.txt
"""
import argparse
import io
import os
import sys
import tempfile
import time
import zlib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from tools.jpeg_timing import per_image_ms, picture, pil_decode      # noqa: E402  the same picture and the same timing loop

FILE_SET = [("256x256 RGB", 256, 256), ("1024x1024 RGB", 1024, 1024)]


def png_bytes(w, h, seed):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(picture(w, h, seed), "RGB").save(buf, "PNG")
    return buf.getvalue()


def idat_stream(data):
    """the concatenated IDAT bodies of a well-formed file"""
    import struct
    pos, out = 8, []
    while pos < len(data):
        n, kind = struct.unpack_from(">I4s", data, pos)
        if kind == b"IDAT":
            out.append(data[pos + 8:pos + 8 + n])
        pos += 12 + n
    return b"".join(out)


def filter_mix(rec):
    import numpy as np
    counts = np.bincount(rec["scan"][::1 + rec["w"] * rec["bpp"]], minlength=5)
    return " ".join(f"{n}:{c}" for n, c in zip(("None", "Sub", "Up", "Avg", "Paeth"), counts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--host-only", action="store_true")
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--seconds", type=float, default=1.0, help="host leg: least duration of a timed window")
    ap.add_argument("--images", type=int, default=256, help="GPU leg: files in the generated 1024 x 1024 folder (4 x as many at 256 x 256)")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default="")
    opt = ap.parse_args()
    from dynamicvectorquantization_amd import data as D
    lines = []

    def say(s=""):
        lines.append(s)
        print(s, flush=True)

    import PIL
    say(f"device PNG decode (tools/png_timing.py); host: {os.cpu_count()} CPUs visible, thread pool of {opt.threads}; Pillow {PIL.__version__}, "
        f"zlib {zlib.ZLIB_RUNTIME_VERSION}")
    say("host leg: ms per image, best of 3 windows; PIL = full decode to a numpy array, host pass = data.decode_png_host, inflate = zlib on the "
        "IDAT stream alone")
    t = str(opt.threads)
    say(f"  {'file':15s} {'bytes':>8s}  {'PIL x1':>8s} {'pass x1':>8s} {'infl x1':>8s} {'ratio':>6s}   {'PIL x' + t:>8s} {'pass x' + t:>8s} "
        f"{'infl x' + t:>8s} {'ratio':>6s}   filters of file 0")
    for label, w, h in FILE_SET:
        datas = [png_bytes(w, h, s) for s in range(4)]
        recs = [D.decode_png_host(d) for d in datas]
        assert all(r is not None for r in recs)
        streams = [idat_stream(d) for d in datas]
        row = []
        for threads in (1, opt.threads):
            a = per_image_ms(pil_decode, datas, threads, opt.seconds)
            b = per_image_ms(D.decode_png_host, datas, threads, opt.seconds)
            c = per_image_ms(zlib.decompress, streams, threads, opt.seconds)
            row += [a, b, c, b / a]
        say(f"  {label:15s} {sum(map(len, datas)) // 4:8d}  {row[0]:8.3f} {row[1]:8.3f} {row[2]:8.3f} {row[3]:6.3f}   {row[4]:8.3f} {row[5]:8.3f} "
            f"{row[6]:8.3f} {row[7]:6.3f}   {filter_mix(recs[0])}")
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
    say()
    say(f"GPU leg: {torch.cuda.get_device_name(0)}, matrix pipes sustain {tf:.0f} TFLOP/s at {mhz:.0f} MHz")
    for (label, w, h), n in zip(FILE_SET, (4 * opt.images, opt.images)):
        with tempfile.TemporaryDirectory(prefix="dvq_png_timing_") as root:
            loader_leg(root, label, w, h, n, opt, say, dev)
    stage_leg(opt, say, dev)


def loader_leg(root, label, w, h, n, opt, say, dev):
    import torch

    from dynamicvectorquantization_amd import data as D
    os.makedirs(os.path.join(root, "c0"))
    distinct = [png_bytes(w, h, s) for s in range(8)]
    for i in range(n):
        with open(os.path.join(root, "c0", f"{i:06d}.png"), "wb") as f:
            f.write(distinct[i % 8])

    def rate(device_png):
        loader = D.GpuBatchLoader(D.ImageFolder(root), opt.batch, dev, size=256, num_workers=opt.threads, device_png=device_png)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        k = 0
        for b in loader:
            k += int(b["image"].shape[0])
        torch.cuda.synchronize()
        return k / (time.perf_counter() - t0)
    rate(False), rate(True)                       # warm: file cache, code objects, pinned pools
    res = {False: [], True: []}
    for _ in range(opt.rounds):
        for on in (False, True):
            res[on].append(rate(on))
    say(f"  GpuBatchLoader over {n} files ({label}), batch {opt.batch}, {opt.threads} host threads, eval transform to 256 x 256; "
        f"{opt.rounds} alternating rounds, images/s:")
    for on in (False, True):
        say(f"    device_png={str(on):5s}  " + "  ".join(f"{v:9.1f}" for v in res[on]) + f"   max {max(res[on]):9.1f}")
    say(f"    on / off: {max(res[True]) / max(res[False]):.3f}")


def stage_leg(opt, say, dev):
    """dvq_png_batch_unfilter alone on buffers that are already resident: what the device stage itself takes"""
    import numpy as np
    import torch

    from dynamicvectorquantization_amd import data as D
    from dynamicvectorquantization_amd.kernels import _p, _s, check, lib
    label, w, h = FILE_SET[1]
    distinct = [D.decode_png_host(png_bytes(w, h, s)) for s in range(8)]
    recs = [distinct[i % 8] for i in range(opt.batch)]
    _, _, _, rgb_len, offs, _ = D.jpeg_batch_layout(recs)
    descs, n, scan_len = D.png_batch_layout(recs, offs)
    scan = torch.from_numpy(np.concatenate([r["scan"] for r in recs])).to(dev)
    desc = torch.from_numpy(np.frombuffer(bytes(descs), dtype=np.uint8).copy()).to(dev)
    rgb = torch.empty(rgb_len, dtype=torch.uint8, device=dev)

    def stage():
        check(lib().dvq_png_batch_unfilter(_p(scan), _p(desc), n, _p(rgb), _s()), "dvq_png_batch_unfilter")
    for _ in range(3):
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
    moved = scan_len + rgb_len
    say(f"  device stage (dvq_png_batch_unfilter), batch of {opt.batch} {label} ({filter_mix(recs[0])}): {best:.4f} ms per batch, min of "
        f"{opt.rounds} x 20 calls = {opt.batch / best * 1e3:.0f} images/s; {moved / 1e6:.1f} MB read and written -> {moved / best / 1e6:.1f} GB/s")


if __name__ == "__main__":
    main()
