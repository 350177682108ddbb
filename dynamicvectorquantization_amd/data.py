"""Input pipeline with the image transforms on the GPU.

Mirrors reference/data/imagenet_base.py:8-64 (ImagePaths: torchvision transforms on PIL images) and
data/build.py:16-90 (DataModuleFromConfig) for the batch dict {"image": fp32 [B,3,S,S] in [-1,1], "class_label": int64 [B], ...}:

    train:  Resize(256) -> RandomCrop(256) -> RandomHorizontalFlip(0.5) -> ToTensor -> Normalize(0.5, 0.5)
    eval:   Resize(256) -> CenterCrop(256) -> Resize((256, 256)) [a no-op] -> ToTensor -> Normalize(0.5, 0.5)

and reference/data/faceshq.py:29-101 (FFHQ), whose training transform is another one:

    train:  RandomResizedCrop(256, scale=(0.75, 1), ratio=(1, 1)) -> RandomHorizontalFlip(0.5) -> ToTensor -> Normalize(0.5, 0.5)

(crop a box of the source, resize the box to 256 x 256: `plan_batch_sizes(boxes=...)`; the same two kernels).  PNG files can be
un-filtered on the GPU as well (device_png=True, "device PNG decode" below).

JPEG decoding runs on host threads (PIL; this image has no rocJPEG) -- or, with device_decode=True, only its Huffman pass does and the
rest runs in csrc/jpeg.hip (see "device JPEG decode" below); the decoded uint8 pixels of a whole batch go to the device in
ONE pinned copy and two kernels (csrc/imgproc.hip) do the rest -- Pillow's antialiased bilinear resampling reproduced bit for
bit in 8-bit fixed point, computed only for the crop window, with flip / ToTensor / Normalize folded into the second pass.  The
reference's 8 PIL workers manage ~1-2 k images/s per node; at >= 330 images/s per GPU x 8 GPUs that would be the bottleneck.

Resampling coefficients (`resample_coeffs`) follow Pillow's src/libImaging/Resample.c (precompute_coeffs with the bilinear
filter, normalize_coeffs_8bpc with PRECISION_BITS = 22); the target size follows torchvision 0.14's Resize(int): shorter side ->
size, longer side -> int(size * long / short).  RandomCrop / flip decisions come from a numpy Generator (the reference's torch
RNG stream is not reproducible across loaders: parity unpinned by construction; tests inject the decisions).
"""
from __future__ import annotations

import ctypes as C
import math
import os
import queue
import struct
import threading
import zlib

import numpy as np
import torch

from . import _lib
from .kernels import _p, _s, check, lib

PRECISION_BITS = 32 - 8 - 2


# ---- host-side arithmetic of the resize (tiny: O(output size) per image) ---------------------------------------------------
def resized_size(w: int, h: int, size: int):
    """torchvision.transforms.Resize(size:int) on a (w, h) image -> (new_w, new_h) (functional._compute_resized_output_size)"""
    short, long = (w, h) if w <= h else (h, w)
    new_short, new_long = size, int(size * long / short)
    return (new_short, new_long) if w <= h else (new_long, new_short)


def resample_coeffs(in_size: int, out_size: int):
    """Pillow's precompute_coeffs (bilinear filter, box = whole axis) + normalize_coeffs_8bpc:
    -> (bounds int32 [out_size, 2] = (first input index, count), coeffs int32 [out_size, ksize], ksize)"""
    scale = in_size / out_size
    filterscale = scale if scale >= 1.0 else 1.0
    support = 1.0 * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    bounds = np.zeros((out_size, 2), dtype=np.int32)
    kk = np.zeros((out_size, ksize), dtype=np.int32)
    ss = 1.0 / filterscale
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = int(center - support + 0.5)
        if xmin < 0:
            xmin = 0
        xmax = int(center + support + 0.5)
        if xmax > in_size:
            xmax = in_size
        xmax -= xmin
        w = []
        ww = 0.0
        for x in range(xmax):
            v = (x + xmin - center + 0.5) * ss
            v = -v if v < 0 else v
            v = 1.0 - v if v < 1.0 else 0.0
            w.append(v)
            ww += v
        for x in range(xmax):
            c = w[x] / ww if ww != 0.0 else w[x]
            kk[xx, x] = int(-0.5 + c * (1 << PRECISION_BITS)) if c < 0 else int(0.5 + c * (1 << PRECISION_BITS))
        bounds[xx] = (xmin, xmax)
    return bounds, kk, ksize


_coeff_cache: dict = {}


def _coeffs_cached(in_size, out_size):
    key = (in_size, out_size)
    hit = _coeff_cache.get(key)
    if hit is None:
        if len(_coeff_cache) > 4096:
            _coeff_cache.clear()
        hit = _coeff_cache[key] = resample_coeffs(in_size, out_size)
    return hit


class _Desc(C.Structure):
    """mirror of ImgDesc in csrc/imgproc.hip"""
    _fields_ = [("src_off", C.c_int64), ("tmp_off", C.c_int64), ("w", C.c_int32), ("h", C.c_int32), ("row0", C.c_int32),
                ("rows", C.c_int32), ("crop_x", C.c_int32), ("crop_y", C.c_int32), ("flip", C.c_int32), ("pad", C.c_int32),
                ("hb_off", C.c_int32), ("hk_off", C.c_int32), ("hks", C.c_int32), ("vb_off", C.c_int32), ("vk_off", C.c_int32),
                ("vks", C.c_int32)]


RRC_SCALE = (0.75, 1.0)       # reference/data/faceshq.py:58: RandomResizedCrop(resolution, scale=(0.75, 1.0), ratio=(1.0, 1.0))


def sample_square_box(w, h, rng, scale=RRC_SCALE):
    """torchvision's RandomResizedCrop.get_params with ratio=(1, 1) on a (w, h) image -> (left, top, bw, bh) in source pixels: up to 10
    tries of area * U(scale), side = int(round(sqrt(target))), accepted when it fits (offsets then drawn uniformly); else that function's
    centred fallback, which for a ratio of exactly 1 is the centred square of the shorter side (the whole image when it is square)."""
    area = w * h
    for _ in range(10):
        side = int(round(math.sqrt(area * float(rng.uniform(scale[0], scale[1])))))
        if 0 < side <= w and 0 < side <= h:
            top, left = int(rng.integers(0, h - side + 1)), int(rng.integers(0, w - side + 1))      # get_params draws i, then j
            return left, top, side, side
    side = min(w, h)
    return (w - side) // 2, (h - side) // 2, side, side


def plan_batch_sizes(sizes, size, crops=None, flips=None, train=False, rng=None, src_offs=None, boxes=None, rrc=None):
    """plan_batch without the pixels: sizes is a list of (w, h) of decoded images that sit (or will sit) packed as uint8 [h][w][3] at
    byte offsets `src_offs` of one buffer (default: back to back).  -> the same dict as plan_batch minus "src", for
    transform_batch_device.  Crop, flip and table logic, and the order of the draws from `rng`, are plan_batch's.
    boxes: per image (left, top, bw, bh) in SOURCE pixels -- crop the box, resize it to size x size (torchvision's resized_crop on a PIL
    image; not Pillow's resize(box=...), which reads pixels outside the box); rrc: a scale range, boxes are then drawn from `rng` by
    sample_square_box (box first, then the flip).  The tables are those of a bw x bh image with left / top added to the bounds, which
    are absolute source indices for the kernels."""
    b = len(sizes)
    descs = (_Desc * b)()
    tabs, tab_len, src_len, tmp_len, max_rows = [], 0, 0, 0, 1
    for i, (w, h) in enumerate(sizes):
        w, h = int(w), int(h)
        left, top, bw, bh = 0, 0, w, h
        nw, nh = resized_size(w, h, size)
        if boxes is not None or rrc is not None:
            left, top, bw, bh = (int(v) for v in boxes[i]) if boxes is not None else sample_square_box(w, h, rng, rrc)
            assert 0 <= left and 0 <= top and 0 < bw and 0 < bh and left + bw <= w and top + bh <= h, "box outside the image"
            nw, nh, cx, cy = size, size, 0, 0
        elif crops is not None:
            cx, cy = crops[i]
        elif train:
            cy, cx = int(rng.integers(0, nh - size + 1)), int(rng.integers(0, nw - size + 1))       # RandomCrop.get_params: i, j
        else:
            cy, cx = int(round((nh - size) / 2.0)), int(round((nw - size) / 2.0))                   # CenterCrop
        flip = bool(flips[i]) if flips is not None else (bool(rng.random() < 0.5) if train else False)
        hb, hk, hks = _coeffs_cached(bw, nw)
        vb, vk, vks = _coeffs_cached(bh, nh)
        hb, hk = hb[cx:cx + size], hk[cx:cx + size]
        vb, vk = vb[cy:cy + size], vk[cy:cy + size]
        if left or top:
            hb, vb = hb + np.array([left, 0], dtype=np.int32), vb + np.array([top, 0], dtype=np.int32)
        row0 = int(vb[:, 0].min())
        rows = int((vb[:, 0] + vb[:, 1]).max()) - row0
        d = descs[i]
        d.src_off = src_len if src_offs is None else int(src_offs[i])
        d.tmp_off, d.w, d.h, d.row0, d.rows = tmp_len, w, h, row0, rows
        d.crop_x, d.crop_y, d.flip = cx, cy, int(flip)
        d.hb_off, d.hk_off, d.hks = tab_len, tab_len + hb.size, hks
        d.vb_off, d.vk_off, d.vks = tab_len + hb.size + hk.size, tab_len + hb.size + hk.size + vb.size, vks
        tabs += [hb.reshape(-1), hk.reshape(-1), vb.reshape(-1), vk.reshape(-1)]
        tab_len += hb.size + hk.size + vb.size + vk.size
        src_len += h * w * 3
        tmp_len += rows * size * 3
        max_rows = max(max_rows, rows)
    return {"desc": np.frombuffer(bytes(descs), dtype=np.uint8).copy(), "tab": np.concatenate(tabs).astype(np.int32),
            "tmp_bytes": tmp_len, "max_rows": max_rows, "batch": b, "size": size}


def plan_batch(images, size, crops=None, flips=None, train=False, rng=None, boxes=None, rrc=None):
    """images: list of uint8 [h,w,3] arrays.  -> dict(src uint8 [bytes], desc uint8 [B * sizeof(ImgDesc)], tab int32 [...],
    tmp_bytes, max_rows): everything the two kernels need, as flat host arrays ready for ONE pinned upload each.
    crops: optional list of (x, y) offsets in the RESIZED image; flips: optional list of bools (else drawn from `rng` when
    train, centre crop / no flip otherwise); boxes / rrc: plan_batch_sizes' crop-a-box-then-resize transform."""
    for im in images:
        assert im.dtype == np.uint8 and im.ndim == 3 and im.shape[2] == 3, "decoded RGB uint8 [h,w,3] expected"
    plan = plan_batch_sizes([(im.shape[1], im.shape[0]) for im in images], size, crops, flips, train, rng, boxes=boxes, rrc=rrc)
    src = np.empty(sum(im.shape[0] * im.shape[1] * 3 for im in images), dtype=np.uint8)
    off = 0
    for im in images:
        n = im.shape[0] * im.shape[1] * 3
        src[off:off + n] = np.ascontiguousarray(im).reshape(-1)
        off += n
    plan["src"] = src
    return plan


def _upload(a, device):
    t = torch.from_numpy(a)
    return t.pin_memory().to(device, non_blocking=True) if device.type == "cuda" else t.to(device)


def transform_batch_device(plan, src, device, out=None):
    """run the two kernels on a planned batch whose decoded pixels are ALREADY on the device: src is the packed uint8 buffer that the
    plan's src_off fields index (decode_batch_gpu's "rgb") -> fp32 [B,3,S,S] on `device` (no synchronisation)"""
    assert C.sizeof(_Desc) == lib().dvq_image_desc_bytes(), "ImgDesc layout mismatch between data.py and imgproc.hip"
    b, s = plan["batch"], plan["size"]
    desc, tab = _upload(plan["desc"], device), _upload(plan["tab"], device)
    tmp = torch.empty(max(1, plan["tmp_bytes"]), dtype=torch.uint8, device=device)
    if out is None:
        out = torch.empty(b, 3, s, s, dtype=torch.float32, device=device)
    check(lib().dvq_image_batch_transform(_p(src), _p(desc), _p(tab), _p(tmp), b, s, plan["max_rows"], _p(out), _s()),
          "dvq_image_batch_transform")
    return out


def transform_batch_gpu(plan, device, out=None):
    """run the two kernels on a planned batch -> fp32 [B,3,S,S] on `device` (no synchronisation)"""
    return transform_batch_device(plan, _upload(plan["src"], device), device, out)


# ---- device JPEG decode (docs/design/23-device-jpeg.md): Huffman pass on the host, the rest in csrc/jpeg.hip --------------------------
class _JpegDesc(C.Structure):
    """mirror of JpegDesc in csrc/jpeg.hip"""
    _fields_ = [("coef_off", C.c_int64), ("plane_off", C.c_int64), ("rgb_off", C.c_int64), ("w", C.c_int32), ("h", C.c_int32),
                ("ncomp", C.c_int32), ("hs", C.c_int32), ("vs", C.c_int32), ("mcux", C.c_int32), ("mcuy", C.c_int32),
                ("idct_item0", C.c_int32), ("idct_items", C.c_int32), ("pix_item0", C.c_int32), ("pix_items", C.c_int32),
                ("pad", C.c_int32 * 3), ("q", C.c_uint16 * 192)]


JPEG_MAX_PIXELS = 1024 * 1024 * 1024 // 4 // 3      # PIL's MAX_IMAGE_PIXELS: larger frames are PIL's to warn about or refuse, as before
JPEG_IDCT_BLOCKS, JPEG_PIX_ITEM = 32, 1024      # work items of the two kernels (IDCT_BLOCKS, PIX_ITEM in csrc/jpeg.hip)


def decode_jpeg_host(path_or_bytes):
    """the host pass on one file: -> coefficient record dict(coef int16 [n], qtab uint16 [ncomp, 64], w, h, ncomp, hs, vs) for
    decode_batch_gpu, or None when the file is not a JPEG this decoder takes (progressive, CMYK, a PNG, a damaged stream ...): the
    caller then uses decode_rgb, as before.  Runs in the library, outside the GIL."""
    if isinstance(path_or_bytes, (bytes, bytearray, memoryview)):
        data = bytes(path_or_bytes)
    else:
        with open(path_or_bytes, "rb") as f:
            data = f.read()
    info = _lib.JpegInfo()
    check(lib().dvq_jpeg_info(data, len(data), C.byref(info)), "dvq_jpeg_info")
    if info.supported != _lib.JPEG_SUPPORTED or info.width * info.height > JPEG_MAX_PIXELS:
        return None
    coef = np.empty(info.coef_count, dtype=np.int16)
    qtab = np.empty((info.components, 64), dtype=np.uint16)
    if lib().dvq_jpeg_entropy_decode(data, len(data), coef.ctypes.data, coef.size, qtab.ctypes.data) != 0:
        return None         # a damaged stream: PIL decides what becomes of it, as it did before
    return {"coef": coef, "qtab": qtab, "w": info.width, "h": info.height, "ncomp": info.components, "hs": info.h_samp[0],
            "vs": info.v_samp[0]}


def jpeg_batch_layout(records):
    """records as decode_batch_gpu takes them -> (descs: ctypes array of _JpegDesc, coef_len in int16 elements, plane_len and rgb_len in
    bytes, offs: byte offset of every image in the RGB buffer, sizes: [(w, h)]): where everything of the batch lies and which share of
    the two kernels' work items each image has"""
    descs = (_JpegDesc * len(records))()
    coef_len = plane_len = rgb_len = idct_items = pix_items = 0
    sizes, offs = [], []
    for i, r in enumerate(records):
        d = descs[i]
        if isinstance(r, np.ndarray):
            assert r.dtype == np.uint8 and r.ndim == 3 and r.shape[2] == 3, "decoded RGB uint8 [h,w,3] expected"
            h, w, ncomp = int(r.shape[0]), int(r.shape[1]), 0
        elif "scan" in r:               # a record of decode_png_host: a slot like a decoded array's, filled by png_batch_layout's launch
            h, w, ncomp = r["h"], r["w"], 0
        else:
            h, w, ncomp, hs, vs = r["h"], r["w"], r["ncomp"], r["hs"], r["vs"]
            assert ncomp in (1, 3) and (hs, vs) in ((1, 1), (2, 1), (2, 2)), "not a record of decode_jpeg_host"
        d.rgb_off, d.w, d.h, d.ncomp = rgb_len, w, h, ncomp
        d.idct_item0, d.pix_item0 = idct_items, pix_items
        if ncomp:
            mcux, mcuy = -(-w // (8 * hs)), -(-h // (8 * vs))
            nblocks = mcux * hs * mcuy * vs + (2 * mcux * mcuy if ncomp == 3 else 0)
            assert r["coef"].size == nblocks * 64 and r["coef"].dtype == np.int16 and r["qtab"].shape == (ncomp, 64)
            d.hs, d.vs, d.mcux, d.mcuy = hs, vs, mcux, mcuy
            d.coef_off, d.plane_off = coef_len, plane_len
            d.idct_items, d.pix_items = -(-nblocks // JPEG_IDCT_BLOCKS), -(-(w * h) // JPEG_PIX_ITEM)
            C.memmove(d.q, r["qtab"].ctypes.data, ncomp * 128)
            coef_len += nblocks * 64
            plane_len += nblocks * 64
            idct_items += d.idct_items
            pix_items += d.pix_items
        sizes.append((w, h))
        offs.append(rgb_len)
        rgb_len += -(-(h * w * 3) // 16) * 16
    assert idct_items < 2 ** 31 and pix_items < 2 ** 31
    return descs, coef_len, plane_len, rgb_len, offs, sizes


# ---- device PNG decode (docs/design/29-device-png.md): chunks, CRCs and inflate on the host, un-filtering in csrc/png.hip ------------
class _PngDesc(C.Structure):
    """mirror of PngDesc in csrc/png.hip"""
    _fields_ = [("scan_off", C.c_int64), ("rgb_off", C.c_int64), ("w", C.c_int32), ("h", C.c_int32), ("bpp", C.c_int32),
                ("pad", C.c_int32)]


PNG_SIGNATURE = b"\x89PNG\r\n\x1a\n"
PNG_BPP = {0: 1, 2: 3, 4: 2, 6: 4}      # colour type -> bytes per pixel at 8 bits: grey, RGB, grey + alpha, RGBA


def _png_decode(data):
    """-> (record or None, reason): parse the chunks, check every CRC, inflate the IDAT stream (bounded), check its length and the
    filter bytes.  Never raises on any bytes."""
    if len(data) < 8 or data[:8] != PNG_SIGNATURE:
        return None, "not a PNG"
    view, n, pos = memoryview(data), len(data), 8
    ihdr, idat, idat_closed, end = None, [], False, False
    while pos < n:
        if pos + 12 > n:
            return None, "truncated chunk"
        length, kind = struct.unpack_from(">I4s", data, pos)
        if pos + 12 + length > n:
            return None, "truncated chunk"
        body = view[pos + 8:pos + 8 + length]
        if zlib.crc32(body, zlib.crc32(kind)) != struct.unpack_from(">I", data, pos + 8 + length)[0]:
            return None, "bad CRC"
        pos += 12 + length
        if ihdr is None:
            if kind != b"IHDR" or length != 13:
                return None, "no IHDR"
            ihdr = struct.unpack(">IIBBBBB", body)
        elif kind == b"IHDR":
            return None, "second IHDR"
        elif kind == b"acTL":
            return None, "APNG"
        elif kind == b"IDAT":
            if idat_closed:
                return None, "IDAT chunks not consecutive"
            idat.append(body)
        elif kind == b"IEND":
            end = True
            break
        elif idat:
            idat_closed = True
    if ihdr is None or not end:
        return None, "truncated file"
    w, h, depth, colour, compression, filt, interlace = ihdr
    if colour == 3:
        return None, "palette"
    if colour not in PNG_BPP:
        return None, "colour type"
    if depth != 8:
        return None, "bit depth"
    if interlace != 0:
        return None, "interlaced"
    if compression != 0 or filt != 0:
        return None, "compression or filter method"
    if w == 0 or h == 0 or w * h > JPEG_MAX_PIXELS:
        return None, "size"
    if not idat:
        return None, "no IDAT"
    bpp = PNG_BPP[colour]
    pitch = 1 + w * bpp
    expected = h * pitch
    z = zlib.decompressobj()
    try:
        raw = z.decompress(idat[0] if len(idat) == 1 else b"".join(idat), expected + 1)      # one byte over: a longer stream shows
    except zlib.error:
        return None, "zlib error"
    if len(raw) != expected:
        return None, "stream length"
    if not z.eof:
        return None, "stream not finished"
    scan = np.frombuffer(raw, dtype=np.uint8)
    if int(scan[::pitch].max()) > 4:
        return None, "filter type"
    return {"scan": scan, "w": w, "h": h, "bpp": bpp}, "ok"


def _file_bytes(path_or_bytes):
    if isinstance(path_or_bytes, (bytes, bytearray, memoryview)):
        return bytes(path_or_bytes)
    with open(path_or_bytes, "rb") as f:
        return f.read()


def decode_png_host(path_or_bytes):
    """the host pass on one file: -> dict(scan uint8 [h * (1 + w * bpp)]: the inflated, still FILTERED scanlines, w, h, bpp) for
    decode_batch_gpu, or None when the file is not a PNG this decoder takes (palette, 16-bit, 1/2/4-bit, interlaced, APNG, a bad CRC, a
    short, long or damaged stream, not a PNG ...): the caller then uses decode_rgb, as before.  Pure Python over zlib, whose crc32 and
    inflate release the GIL on large buffers.  The length and the filter bytes are checked here, so the device never reads outside
    the buffer and never meets a filter type above 4."""
    return _png_decode(_file_bytes(path_or_bytes))[0]


def png_info(data):
    """(supported, reason) for the bytes of a file: why decode_png_host leaves it to PIL ("ok" when it does not)"""
    rec, reason = _png_decode(bytes(data))
    return rec is not None, reason


def png_batch_layout(records, offs):
    """records as decode_batch_gpu takes them and their byte offsets in the RGB buffer (jpeg_batch_layout's) -> (descs: ctypes array of
    _PngDesc, one per PNG record, in order; their number; scan_len: bytes of the batch's scanlines back to back)"""
    pngs = [(r, off) for r, off in zip(records, offs) if not isinstance(r, np.ndarray) and "scan" in r]
    descs = (_PngDesc * max(1, len(pngs)))()
    scan_len = 0
    for d, (r, off) in zip(descs, pngs):
        assert r["bpp"] in (1, 2, 3, 4) and r["w"] > 0 and r["h"] > 0, "not a record of decode_png_host"
        assert r["scan"].dtype == np.uint8 and r["scan"].size == r["h"] * (1 + r["w"] * r["bpp"]), "scanline buffer of the wrong length"
        d.scan_off, d.rgb_off, d.w, d.h, d.bpp = scan_len, off, r["w"], r["h"], r["bpp"]
        scan_len += r["scan"].size
    return descs, len(pngs), scan_len


def example_record(ex):
    """what decode_batch_gpu takes for a dataset example: its JPEG or PNG record, else its decoded pixels"""
    return ex["jpeg"] if "jpeg" in ex else (ex["png"] if "png" in ex else ex["image_u8"])


def decode_batch_gpu(records, device):
    """records: per image a coefficient record of decode_jpeg_host, a scanline record of decode_png_host, or a decoded uint8 [h,w,3]
    array (what decode_rgb gave for a file the host passes left alone).  One pinned upload of the batch's coefficients, one of its
    descriptors, two launches (dvq_jpeg_batch_decode); for PNG records one pinned upload of the scanlines, one of their descriptors, one
    launch (dvq_png_batch_unfilter) -> dict(rgb: uint8 device buffer with every image packed [h][w][3] at a 16-byte aligned offset, offs:
    the byte offsets, sizes: [(w, h)]) -- plan_batch_sizes and transform_batch_device take it from there.  Host-decoded images are copied
    into their slots of the same buffer.  No synchronisation."""
    device = torch.device(device)
    if device.type != "cuda":
        raise _lib.DvqError("decode_batch_gpu needs a GPU (no CPU fallback)")
    assert C.sizeof(_JpegDesc) == lib().dvq_jpeg_desc_bytes(), "JpegDesc layout mismatch between data.py and jpeg.hip"
    descs, coef_len, plane_len, rgb_len, offs, sizes = jpeg_batch_layout(records)
    rgb = torch.empty(max(16, rgb_len), dtype=torch.uint8, device=device)
    if coef_len:
        coef = torch.empty(coef_len, dtype=torch.int16, pin_memory=True)
        host = coef.numpy()
        for d, r in zip(descs, records):
            if d.ncomp:
                host[d.coef_off:d.coef_off + r["coef"].size] = r["coef"]
        coef = coef.to(device, non_blocking=True)
        desc = _upload(np.frombuffer(bytes(descs), dtype=np.uint8).copy(), device)
        planes = torch.empty(plane_len, dtype=torch.uint8, device=device)
        check(lib().dvq_jpeg_batch_decode(_p(coef), _p(desc), len(records), _p(planes), _p(rgb), _s()), "dvq_jpeg_batch_decode")
    pdescs, npng, scan_len = png_batch_layout(records, offs)
    if npng:
        assert C.sizeof(_PngDesc) == lib().dvq_png_desc_bytes(), "PngDesc layout mismatch between data.py and png.hip"
        scan = torch.empty(scan_len, dtype=torch.uint8, pin_memory=True)
        host = scan.numpy()
        for d, r in zip(pdescs, (r for r in records if not isinstance(r, np.ndarray) and "scan" in r)):
            host[d.scan_off:d.scan_off + r["scan"].size] = r["scan"]
        scan = scan.to(device, non_blocking=True)
        pdesc = _upload(np.frombuffer(bytes(pdescs), dtype=np.uint8)[:npng * C.sizeof(_PngDesc)].copy(), device)
        check(lib().dvq_png_batch_unfilter(_p(scan), _p(pdesc), npng, _p(rgb), _s()), "dvq_png_batch_unfilter")
    for off, r in zip(offs, records):
        if isinstance(r, np.ndarray):
            rgb[off:off + r.size].copy_(torch.from_numpy(np.array(r, dtype=np.uint8, order="C").reshape(-1)))
    return {"rgb": rgb, "offs": offs, "sizes": sizes}


# ---- datasets / loader (data/imagenet_base.py ImagePaths, data/imagenet.py, data/build.py) ----------------------------------------
def decode_rgb(path) -> np.ndarray:
    """PIL decode -> uint8 [h,w,3] (imagenet_base.py:50-53: non-RGB images are converted)"""
    from PIL import Image
    with Image.open(path) as im:
        if im.mode != "RGB":
            im = im.convert("RGB")
        return np.asarray(im, dtype=np.uint8)


class ImagePaths:
    """file list + labels; `__getitem__` returns the DECODED image and its labels -- the transform happens per batch on the GPU"""

    def __init__(self, paths, labels=None, is_train=False, device_decode=False, device_png=False):
        self.paths = list(paths)
        self.labels = dict(labels or {})
        self.labels["file_path_"] = self.paths
        self.is_train = is_train
        self.device_decode = device_decode      # hand over coefficient records ("jpeg") where the host pass takes the file
        self.device_png = device_png            # hand over scanline records ("png") where decode_png_host takes the file

    def __len__(self):
        return len(self.paths)

    def __getitem__(self, i):
        return self.example(i, self.device_decode, self.device_png)

    def example(self, i, device_decode=False, device_png=False):
        rec = decode_jpeg_host(self.paths[i]) if device_decode else None
        ex = {"jpeg": rec} if rec is not None else None
        if ex is None and device_png:
            rec = decode_png_host(self.paths[i])
            ex = {"png": rec} if rec is not None else None
        if ex is None:
            ex = {"image_u8": decode_rgb(self.paths[i])}
        for k, v in self.labels.items():
            ex[k] = v[i]
        return ex


class ImageFolder(ImagePaths):
    """<root>/<class dir>/<image>: class_label = index of the class directory in sorted order (data/imagenet.py:75-82: labels
    are the indices of np.unique(synsets)), relpath, synset"""
    EXTS = (".jpeg", ".jpg", ".png", ".bmp", ".webp")

    def __init__(self, root, is_train=False, limit=None, device_decode=False, device_png=False):
        classes = sorted(d for d in os.listdir(root) if os.path.isdir(os.path.join(root, d)))
        rel, syn = [], []
        for c in classes:
            for f in sorted(os.listdir(os.path.join(root, c))):
                if f.lower().endswith(self.EXTS):
                    rel.append(os.path.join(c, f))
                    syn.append(c)
        if limit:
            rel, syn = rel[:limit], syn[:limit]
        idx = {c: i for i, c in enumerate(sorted(set(syn)))}
        labels = {"relpath": np.array(rel), "synsets": np.array(syn), "class_label": np.array([idx[s] for s in syn], dtype=np.int64)}
        super().__init__([os.path.join(root, r) for r in rel], labels, is_train, device_decode, device_png)


def _imagenet_root(split):
    root = os.environ.get("DVQ_IMAGENET_ROOT")
    if not root:
        raise FileNotFoundError("set DVQ_IMAGENET_ROOT to a directory holding train/ and val/ class folders "
                                "(the reference's data/default.py points at its own cluster path)")
    return os.path.join(root, split)


class ImageNetTrain(ImageFolder):
    """data/imagenet.py:ImageNetTrain(config={is_eval, size}) on $DVQ_IMAGENET_ROOT/train"""

    def __init__(self, config=None):
        self.config = dict(config or {})
        super().__init__(_imagenet_root("train"), is_train=not self.config.get("is_eval", False))


class ImageNetValidation(ImageFolder):
    def __init__(self, config=None):
        self.config = dict(config or {})
        super().__init__(_imagenet_root("val"), is_train=False)


class FFHQ(ImagePaths):
    """data/faceshq.py:FFHQ(split, resolution, is_eval): <root>/FFHQ/<name> for the names listed in <root>/assets/ffhqtrain.txt
    (split "train") or ffhqvalidation.txt ("val"); "trainval" lists the folder.  Examples carry "image" only (no class keys).  The
    training split asks for the reference's RandomResizedCrop(resolution, scale=(0.75, 1), ratio=(1, 1)) + flip through
    `transform_kind` (GpuBatchLoader hands it to the planner); every other use gets the eval transform.  `root` comes from the YAML or
    a dotlist override (data.params.train.params.root=...)."""
    EXTS = (".jpg", ".jpeg", ".png", ".ppm", ".bmp", ".pgm", ".tif", ".tiff", ".webp")       # torchvision's IMG_EXTENSIONS
    SPLITS = ("train", "val", "trainval")

    def __init__(self, split="train", resolution=256, is_eval=False, root=None, train_list_file=None, val_list_file=None,
                 device_decode=False, device_png=False):
        if split not in self.SPLITS:
            raise ValueError(f"Unknown split {split}. Valid splits are {', '.join(self.SPLITS)}.")
        if not root or not os.path.isdir(os.path.join(root, "FFHQ")):
            raise FileNotFoundError(f"FFHQ: no image folder {os.path.join(str(root), 'FFHQ')}: set the dataset's `root` key (YAML, or "
                                    f"data.params.<split>.params.root=DIR on the command line) to a directory holding FFHQ/ and "
                                    f"assets/ffhqtrain.txt, assets/ffhqvalidation.txt (the reference points at its own cluster path)")
        folder = os.path.join(root, "FFHQ")
        if split == "trainval":
            names = [f for f in os.listdir(folder) if f.lower().endswith(self.EXTS)]
        else:
            listfile = (train_list_file or os.path.join(root, "assets", "ffhqtrain.txt")) if split == "train" else \
                (val_list_file or os.path.join(root, "assets", "ffhqvalidation.txt"))
            with open(listfile) as f:
                names = [line.strip() for line in f.readlines() if line.strip()]
        self.split, self.resolution = split, resolution
        train = split == "train" and not is_eval
        self.transform_kind = "random_resized_crop" if train else None
        super().__init__([os.path.join(folder, name) for name in names], None, train, device_decode, device_png)


class GpuBatchLoader:
    """iterates a dataset in batches: `num_workers` host threads decode, the transforms of a whole batch run on the GPU, batches
    are produced `prefetch` ahead of the consumer on a side stream"""

    def __init__(self, dataset, batch_size, device, size=256, shuffle=False, num_workers=8, seed=0, drop_last=True, prefetch=2,
                 device_decode=False, device_png=False):
        self.ds, self.bs, self.device, self.size = dataset, batch_size, torch.device(device), size
        if device_decode and not hasattr(dataset, "example"):
            raise TypeError("device_decode needs a dataset with example(i, device_decode) (data.ImagePaths and its subclasses)")
        if device_png and not hasattr(dataset, "example"):
            raise TypeError("device_png needs a dataset with example(i, device_decode, device_png) (data.ImagePaths and its subclasses)")
        self.device_decode, self.device_png = device_decode, device_png
        # a dataset may ask for another training transform than Resize + RandomCrop (data.FFHQ: "random_resized_crop")
        self.rrc = RRC_SCALE if getattr(dataset, "transform_kind", None) == "random_resized_crop" else None
        self.shuffle, self.workers, self.drop_last, self.prefetch = shuffle, max(1, num_workers), drop_last, prefetch
        self.rng = np.random.default_rng(seed)
        self.train = bool(getattr(dataset, "is_train", False))

    def __len__(self):
        n = len(self.ds)
        return n // self.bs if self.drop_last else -(-n // self.bs)

    def _batch(self, idxs, pool):
        # device_decode: ask the dataset for coefficient records; a dataset that was built with device_decode hands them over anyway
        if self.device_png:
            get = lambda i: self.ds.example(i, self.device_decode, True)         # noqa: E731
        else:
            get = (lambda i: self.ds.example(i, True)) if self.device_decode else self.ds.__getitem__
        ex = list(pool.map(get, idxs))
        if any("jpeg" in e or "png" in e for e in ex):
            dec = decode_batch_gpu([example_record(e) for e in ex], self.device)
            plan = plan_batch_sizes(dec["sizes"], self.size, train=self.train, rng=self.rng, src_offs=dec["offs"], rrc=self.rrc)
            out = {"image": transform_batch_device(plan, dec["rgb"], self.device)}
        else:
            plan = plan_batch([e["image_u8"] for e in ex], self.size, train=self.train, rng=self.rng, rrc=self.rrc)
            out = {"image": transform_batch_gpu(plan, self.device)}
        keys = [k for k in ex[0] if k not in ("image_u8", "jpeg", "png")]
        for k in keys:
            vals = [e[k] for e in ex]
            out[k] = torch.as_tensor(np.asarray(vals)).to(self.device) if np.asarray(vals).dtype.kind in "iuf" else vals
        return out

    def __iter__(self):
        from concurrent.futures import ThreadPoolExecutor
        order = self.rng.permutation(len(self.ds)) if self.shuffle else np.arange(len(self.ds))
        batches = [order[i:i + self.bs] for i in range(0, len(order), self.bs)]
        if self.drop_last and batches and len(batches[-1]) < self.bs:
            batches.pop()
        q: queue.Queue = queue.Queue(maxsize=self.prefetch)
        stream = torch.cuda.Stream(self.device) if self.device.type == "cuda" else None

        def producer():
            try:
                with ThreadPoolExecutor(self.workers) as pool:
                    for idxs in batches:
                        if stream is not None:
                            with torch.cuda.stream(stream):
                                b = self._batch(idxs, pool)
                                ev = torch.cuda.Event()
                                ev.record(stream)
                        else:
                            b, ev = self._batch(idxs, pool), None
                        q.put((b, ev))
                q.put(None)
            except BaseException as e:      # noqa: BLE001 -- surfaced in the consumer thread
                q.put(e)

        threading.Thread(target=producer, daemon=True).start()
        while True:
            item = q.get()
            if item is None:
                return
            if isinstance(item, BaseException):
                raise item
            b, ev = item
            if ev is not None:
                cur = torch.cuda.current_stream(self.device)
                cur.wait_event(ev)
                # the batch was allocated on the producer's stream: tell the caching allocator that the consumer's stream
                # reads it too, so that a dropped batch is not handed back to the producer (and overwritten by the next
                # transform) while the training stream, which runs steps behind the host, still reads it
                for t in b.values():
                    if torch.is_tensor(t) and t.is_cuda:
                        t.record_stream(cur)
            yield b


class DataModuleFromConfig:
    """data/build.py:16-90: {batch_size, train, validation, test, num_workers} -> *_dataloader() yielding GPU-resident batch dicts"""

    def __init__(self, batch_size, train=None, validation=None, test=None, wrap=False, num_workers=None, train_val=False,
                 device="cuda", size=256, device_decode=False, device_png=False):
        from .config import instantiate_from_config
        self.device_decode, self.device_png = device_decode, device_png
        self.batch_size = batch_size
        self.num_workers = num_workers if num_workers is not None else batch_size * 2
        self.dataset_configs = {k: v for k, v in (("train", train), ("validation", validation), ("test", test)) if v is not None}
        self.device, self.size = device, size
        self.datasets = {k: instantiate_from_config(v) for k, v in self.dataset_configs.items()}
        for k, d in self.datasets.items():
            print("dataset: ", k, len(d))

    def prepare_data(self):
        pass

    def _loader(self, split, shuffle):
        return GpuBatchLoader(self.datasets[split], self.batch_size, self.device, self.size, shuffle=shuffle,
                              num_workers=min(self.num_workers, 32), device_decode=self.device_decode, device_png=self.device_png)

    def train_dataloader(self):
        return self._loader("train", True)

    def val_dataloader(self):
        return self._loader("validation", False)

    def test_dataloader(self):
        return self._loader("test", False)
