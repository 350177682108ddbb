"""Input pipeline with the image transforms on the GPU.

Mirrors reference/data/imagenet_base.py:8-64 (ImagePaths: torchvision transforms on PIL images) and
data/build.py:16-90 (DataModuleFromConfig) for the batch dict {"image": fp32 [B,3,S,S] in [-1,1], "class_label": int64 [B], ...}:

    train:  Resize(256) -> RandomCrop(256) -> RandomHorizontalFlip(0.5) -> ToTensor -> Normalize(0.5, 0.5)
    eval:   Resize(256) -> CenterCrop(256) -> Resize((256, 256)) [a no-op] -> ToTensor -> Normalize(0.5, 0.5)

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
import threading

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


def plan_batch_sizes(sizes, size, crops=None, flips=None, train=False, rng=None, src_offs=None):
    """plan_batch without the pixels: sizes is a list of (w, h) of decoded images that sit (or will sit) packed as uint8 [h][w][3] at
    byte offsets `src_offs` of one buffer (default: back to back).  -> the same dict as plan_batch minus "src", for
    transform_batch_device.  Crop, flip and table logic, and the order of the draws from `rng`, are plan_batch's."""
    b = len(sizes)
    descs = (_Desc * b)()
    tabs, tab_len, src_len, tmp_len, max_rows = [], 0, 0, 0, 1
    for i, (w, h) in enumerate(sizes):
        w, h = int(w), int(h)
        nw, nh = resized_size(w, h, size)
        if crops is not None:
            cx, cy = crops[i]
        elif train:
            cy, cx = int(rng.integers(0, nh - size + 1)), int(rng.integers(0, nw - size + 1))       # RandomCrop.get_params: i, j
        else:
            cy, cx = int(round((nh - size) / 2.0)), int(round((nw - size) / 2.0))                   # CenterCrop
        flip = bool(flips[i]) if flips is not None else (bool(rng.random() < 0.5) if train else False)
        hb, hk, hks = _coeffs_cached(w, nw)
        vb, vk, vks = _coeffs_cached(h, nh)
        hb, hk = hb[cx:cx + size], hk[cx:cx + size]
        vb, vk = vb[cy:cy + size], vk[cy:cy + size]
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


def plan_batch(images, size, crops=None, flips=None, train=False, rng=None):
    """images: list of uint8 [h,w,3] arrays.  -> dict(src uint8 [bytes], desc uint8 [B * sizeof(ImgDesc)], tab int32 [...],
    tmp_bytes, max_rows): everything the two kernels need, as flat host arrays ready for ONE pinned upload each.
    crops: optional list of (x, y) offsets in the RESIZED image; flips: optional list of bools (else drawn from `rng` when
    train, centre crop / no flip otherwise)."""
    for im in images:
        assert im.dtype == np.uint8 and im.ndim == 3 and im.shape[2] == 3, "decoded RGB uint8 [h,w,3] expected"
    plan = plan_batch_sizes([(im.shape[1], im.shape[0]) for im in images], size, crops, flips, train, rng)
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


def decode_batch_gpu(records, device):
    """records: per image a coefficient record of decode_jpeg_host, or a decoded uint8 [h,w,3] array (what decode_rgb gave for a file
    the host pass left alone).  One pinned upload of the batch's coefficients, one of its descriptors, two launches
    (dvq_jpeg_batch_decode) -> dict(rgb: uint8 device buffer with every image packed [h][w][3] at a 16-byte aligned offset, offs: the
    byte offsets, sizes: [(w, h)]) -- plan_batch_sizes and transform_batch_device take it from there.  Host-decoded images are copied
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

    def __init__(self, paths, labels=None, is_train=False, device_decode=False):
        self.paths = list(paths)
        self.labels = dict(labels or {})
        self.labels["file_path_"] = self.paths
        self.is_train = is_train
        self.device_decode = device_decode      # hand over coefficient records ("jpeg") where the host pass takes the file

    def __len__(self):
        return len(self.paths)

    def __getitem__(self, i):
        return self.example(i, self.device_decode)

    def example(self, i, device_decode=False):
        rec = decode_jpeg_host(self.paths[i]) if device_decode else None
        ex = {"jpeg": rec} if rec is not None else {"image_u8": decode_rgb(self.paths[i])}
        for k, v in self.labels.items():
            ex[k] = v[i]
        return ex


class ImageFolder(ImagePaths):
    """<root>/<class dir>/<image>: class_label = index of the class directory in sorted order (data/imagenet.py:75-82: labels
    are the indices of np.unique(synsets)), relpath, synset"""
    EXTS = (".jpeg", ".jpg", ".png", ".bmp", ".webp")

    def __init__(self, root, is_train=False, limit=None, device_decode=False):
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
        super().__init__([os.path.join(root, r) for r in rel], labels, is_train, device_decode)


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


class GpuBatchLoader:
    """iterates a dataset in batches: `num_workers` host threads decode, the transforms of a whole batch run on the GPU, batches
    are produced `prefetch` ahead of the consumer on a side stream"""

    def __init__(self, dataset, batch_size, device, size=256, shuffle=False, num_workers=8, seed=0, drop_last=True, prefetch=2,
                 device_decode=False):
        self.ds, self.bs, self.device, self.size = dataset, batch_size, torch.device(device), size
        if device_decode and not hasattr(dataset, "example"):
            raise TypeError("device_decode needs a dataset with example(i, device_decode) (data.ImagePaths and its subclasses)")
        self.device_decode = device_decode
        self.shuffle, self.workers, self.drop_last, self.prefetch = shuffle, max(1, num_workers), drop_last, prefetch
        self.rng = np.random.default_rng(seed)
        self.train = bool(getattr(dataset, "is_train", False))

    def __len__(self):
        n = len(self.ds)
        return n // self.bs if self.drop_last else -(-n // self.bs)

    def _batch(self, idxs, pool):
        # device_decode: ask the dataset for coefficient records; a dataset that was built with device_decode hands them over anyway
        ex = list(pool.map((lambda i: self.ds.example(i, True)) if self.device_decode else self.ds.__getitem__, idxs))
        if any("jpeg" in e for e in ex):
            dec = decode_batch_gpu([e["jpeg"] if "jpeg" in e else e["image_u8"] for e in ex], self.device)
            plan = plan_batch_sizes(dec["sizes"], self.size, train=self.train, rng=self.rng, src_offs=dec["offs"])
            out = {"image": transform_batch_device(plan, dec["rgb"], self.device)}
        else:
            plan = plan_batch([e["image_u8"] for e in ex], self.size, train=self.train, rng=self.rng)
            out = {"image": transform_batch_gpu(plan, self.device)}
        keys = [k for k in ex[0] if k not in ("image_u8", "jpeg")]
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
                 device="cuda", size=256, device_decode=False):
        from .config import instantiate_from_config
        self.device_decode = device_decode
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
                              num_workers=min(self.num_workers, 32), device_decode=self.device_decode)

    def train_dataloader(self):
        return self._loader("train", True)

    def val_dataloader(self):
        return self._loader("validation", False)

    def test_dataloader(self):
        return self._loader("test", False)
