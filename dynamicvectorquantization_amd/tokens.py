"""Token shards: the frozen DQ-VAE's output stored once, and stage 2 trained / scored from it (docs/design/16-token-shards.md).

A token set is a directory with `meta.json` and `tokens-00000.npy`, `tokens-00001.npy`, ... (`tokens-pIIII-NNNNN.npy` when it was
written in parts).  Every file is ONE uncompressed .npy of fixed-size records (`record_dtype`), so `np.load(mmap_mode="r")` gives
random access without an index.  One record = one view of one image: the full [fhw, fhw] code map as uint16, the grain map as a
bitmap (bit c % 32 of word c // 32 = coarse cell c is fine), its popcount, label, source image index, view number.  Records are stored
image-major: record r = image r // views, view r % views.

  * TokenShardWriter / finalize_parts   append batches, roll files at shard_size, temporary name + rename, meta.json LAST
  * TokenShardDataset                   opens and checks a set (a set without meta.json is incomplete and refused); check_model()
  * TokenBatchLoader                    data.GpuBatchLoader's shape: producer thread, `prefetch` batches ahead on a side stream; per
                                        batch one pinned upload and one dvq_tokens_unpack launch, row lengths from the host's popcount
                                        of the bitmaps -- no device-to-host read anywhere

  * tokenize_batches                    encode -> dvq_tokens_pack -> writer, one synchronisation per batch

The format half (writer, dataset, plan_epoch) is numpy only, and torch / libdvq_hip are imported inside the functions that launch
kernels: importing this module needs neither the library nor a GPU.
"""
from __future__ import annotations

import hashlib
import json
import os
import queue
import threading

import numpy as np

FORMAT_VERSION = 1
META = "meta.json"
STREAM_KEYS = ("coarse_content", "fine_content", "coarse_position", "fine_position", "coarse_segment", "fine_segment")
FEATURE_ROUTER = "feature-router"


class TokenSetError(ValueError):
    """a token set that is incomplete, damaged, of an unknown version, or made by another first stage"""


# ---- record layout / bitmap arithmetic ------------------------------------------------------------------------------------------------
def grain_words(hw1: int) -> int:
    return (int(hw1) * int(hw1) + 31) // 32


def record_dtype(hw1: int, hw2: int) -> np.dtype:
    fhw = int(hw1) * int(hw2)
    return np.dtype([("codes", "<u2", (fhw, fhw)), ("grain", "<u4", (grain_words(hw1),)), ("n_fine_cells", "<u2"), ("label", "<i4"),
                     ("source", "<i4"), ("view", "u1")])


def pack_grain_bits(grain) -> np.ndarray:
    """grain [N, hw1, hw1] (1 = fine, anything else coarse) -> uint32 [N, ceil(hw1^2 / 32)], unused high bits 0"""
    g = np.asarray(grain)
    n, ncell = g.shape[0], g.shape[1] * g.shape[2]
    w = (ncell + 31) // 32
    flat = np.zeros((n, w * 32), dtype=np.uint8)
    flat[:, :ncell] = g.reshape(n, ncell) == 1
    return np.ascontiguousarray(np.packbits(flat, axis=1, bitorder="little")).view("<u4").reshape(n, w)


def unpack_grain_bits(bits, hw1: int) -> np.ndarray:
    """uint32 [N, W] -> int64 [N, hw1, hw1] of 0 / 1"""
    b = np.ascontiguousarray(np.asarray(bits, dtype="<u4"))
    n = b.shape[0]
    flat = np.unpackbits(b.view(np.uint8).reshape(n, -1), axis=1, bitorder="little")
    return flat[:, :hw1 * hw1].astype(np.int64).reshape(n, hw1, hw1)


def popcount_rows(bits) -> np.ndarray:
    """uint32 [N, W] -> int64 [N]: set bits per row"""
    b = np.ascontiguousarray(np.asarray(bits, dtype="<u4"))
    return np.unpackbits(b.view(np.uint8).reshape(b.shape[0], -1), axis=1).sum(axis=1).astype(np.int64)


def row_lengths(n_fine_cells, hw1: int, hw2: int):
    """(Lc, Lf) of a batch from its fine-cell counts: the permuter's row lengths, longest stream + 1 for its <eos>"""
    n = np.asarray(n_fine_cells, dtype=np.int64)
    return int(hw1 * hw1 - n.min()) + 1, int(n.max()) * int(hw2) * int(hw2) + 1


def batch_lengths(bits, stored_counts, hw1: int, hw2: int):
    """fine cells per record by popcount of the gathered bitmaps, checked against the stored counts -> (n int64 [B], Lc, Lf)"""
    n = popcount_rows(bits)
    stored = np.asarray(stored_counts, dtype=np.int64)
    if not np.array_equal(n, stored):
        i = int(np.nonzero(n != stored)[0][0])
        raise TokenSetError(f"record {i} of the batch stores n_fine_cells = {int(stored[i])}, its bitmap has {int(n[i])} fine cells")
    return (n,) + row_lengths(n, hw1, hw2)


def fingerprint_arrays(codebook_weight, threshold) -> str:
    """sha256 over the bytes of the codebook weight (fp32) and of the router's threshold (fp64), or "feature-router" without one"""
    if threshold is None:
        return FEATURE_ROUTER
    h = hashlib.sha256()
    h.update(np.ascontiguousarray(np.asarray(codebook_weight, dtype="<f4")).tobytes())
    h.update(np.asarray(float(threshold), dtype="<f8").tobytes())
    return h.hexdigest()


def first_stage_fingerprint(first_stage) -> str:
    """fingerprint_arrays of a DualGrainVQModel: the quantiser's stored codebook weight (quantize.codebook_of) and the fixed entropy router's fine_grain_threshold"""
    router = getattr(getattr(first_stage, "encoder", None), "router", None)
    thr = getattr(router, "fine_grain_threshold", None)
    if thr is None:
        return FEATURE_ROUTER
    from .quantize import codebook_of
    w = codebook_of(first_stage.quantize)[0]
    return fingerprint_arrays(w.detach().float().cpu().numpy(), thr)


def describe_model(model) -> dict:
    """what a token set must agree with: a Dualformer (hw1 / hw2 from its permuter, first_stage_model) or a bare first stage given
    together with hw1 / hw2 attributes"""
    fs = getattr(model, "first_stage_model", model)
    from .quantize import codebook_of
    return {"hw1": int(model.hw1), "hw2": int(model.hw2), "codebook_size": codebook_of(fs.quantize)[1],
            "fingerprint": first_stage_fingerprint(fs)}


# ---- writer ----------------------------------------------------------------------------------------------------------------------------
def _write_json(path, obj):
    tmp = path + ".tmp"
    with open(tmp, "w", encoding="utf-8") as f:
        json.dump(obj, f, indent=1, sort_keys=True)
        f.write("\n")
    os.replace(tmp, path)


def _part_name(part):
    return f"part-{part[0]:04d}.json"


class TokenShardWriter:
    """appends record batches to <out>/tokens-NNNNN.npy, `shard_size` records per file (temporary name, then rename); close() writes
    meta.json last.  part = (i, n): files are tokens-pIIII-NNNNN.npy and close() writes part-IIII.json instead -- finalize_parts() turns
    n complete parts into a set."""

    def __init__(self, out_dir, hw1, hw2, codebook_size, views, shard_size=65536, compute_dtype="bf16", fingerprint=FEATURE_ROUTER,
                 dataset=None, part=None):
        if int(shard_size) <= 0:
            raise ValueError("shard_size must be positive")
        if not 0 < int(codebook_size) <= 65536:
            raise ValueError(f"codebook_size {codebook_size} does not fit uint16 codes")
        self.out, self.hw1, self.hw2 = str(out_dir), int(hw1), int(hw2)
        self.dtype = record_dtype(hw1, hw2)
        self.shard_size, self.part = int(shard_size), (int(part[0]), int(part[1])) if part is not None else None
        self.header = {"version": FORMAT_VERSION, "hw1": self.hw1, "hw2": self.hw2, "codebook_size": int(codebook_size),
                       "views": [str(v) for v in views], "n_views": len(views), "compute_dtype": str(compute_dtype),
                       "fingerprint": str(fingerprint), "dataset": dataset if dataset is not None else {}}
        if not views:
            raise ValueError("a token set stores at least one view per image")
        os.makedirs(self.out, exist_ok=True)
        if os.path.exists(os.path.join(self.out, META)):
            raise TokenSetError(f"{self.out} already holds a complete token set")
        self.files, self._buf, self._fill = [], np.zeros(self.shard_size, dtype=self.dtype), 0

    def _name(self, i):
        return f"tokens-p{self.part[0]:04d}-{i:05d}.npy" if self.part is not None else f"tokens-{i:05d}.npy"

    def _flush(self):
        if self._fill == 0:
            return
        name = self._name(len(self.files))
        path = os.path.join(self.out, name)
        with open(path + ".tmp", "wb") as f:
            np.save(f, self._buf[:self._fill], allow_pickle=False)
        os.replace(path + ".tmp", path)
        self.files.append({"name": name, "records": int(self._fill)})
        self._fill = 0

    def append_records(self, rec):
        rec = np.asarray(rec)
        if rec.dtype != self.dtype:
            raise TypeError(f"records of dtype {rec.dtype}, this set stores {self.dtype}")
        i = 0
        while i < rec.shape[0]:
            n = min(rec.shape[0] - i, self.shard_size - self._fill)
            self._buf[self._fill:self._fill + n] = rec[i:i + n]
            self._fill += n
            i += n
            if self._fill == self.shard_size:
                self._flush()

    def append(self, codes, grain_bits, n_fine_cells, label, source, view):
        """one batch of records from host arrays: codes [n, fhw * fhw] or [n, fhw, fhw], grain_bits [n, W], the rest [n]"""
        n = int(np.asarray(codes).shape[0])
        rec = np.zeros(n, dtype=self.dtype)
        rec["codes"] = np.asarray(codes).reshape((n,) + self.dtype["codes"].shape)
        rec["grain"] = np.asarray(grain_bits).reshape(n, -1)
        rec["n_fine_cells"], rec["label"], rec["source"], rec["view"] = n_fine_cells, label, source, view
        self.append_records(rec)

    def close(self):
        self._flush()
        if self.part is not None:
            _write_json(os.path.join(self.out, _part_name(self.part)), dict(self.header, part=list(self.part), files=self.files))
            return None
        meta = dict(self.header, files=self.files, records=sum(f["records"] for f in self.files))
        _write_json(os.path.join(self.out, META), meta)
        return meta


def finalize_parts(out_dir) -> dict:
    """meta.json from the part-IIII.json files of `out_dir`: every part 0 .. n-1 present, all made with the same first stage, grid, views
    and dataset; whole images only (records divisible by the views)"""
    out_dir = str(out_dir)
    names = sorted(f for f in os.listdir(out_dir) if f.startswith("part-") and f.endswith(".json"))
    if not names:
        raise TokenSetError(f"{out_dir}: no part-*.json to finalize")
    parts = []
    for f in names:
        with open(os.path.join(out_dir, f), "r", encoding="utf-8") as fh:
            parts.append(json.load(fh))
    n = int(parts[0]["part"][1])
    have = sorted(int(p["part"][0]) for p in parts)
    if have != list(range(n)):
        raise TokenSetError(f"{out_dir}: parts {have} present, 0 .. {n - 1} needed")
    keys = ("version", "hw1", "hw2", "codebook_size", "views", "n_views", "compute_dtype", "fingerprint", "dataset")
    parts.sort(key=lambda p: int(p["part"][0]))
    for p in parts[1:]:
        for k in keys:
            if p[k] != parts[0][k] or int(p["part"][1]) != n:
                raise TokenSetError(f"{out_dir}: part {p['part'][0]} disagrees with part 0 on '{k}': {p[k]!r} != {parts[0][k]!r}")
    files = [f for p in parts for f in p["files"]]
    for f in files:
        if not os.path.exists(os.path.join(out_dir, f["name"])):
            raise TokenSetError(f"{out_dir}: {f['name']} is missing")
    meta = {k: parts[0][k] for k in keys}
    meta.update(files=files, records=sum(f["records"] for f in files), parts=n)
    if meta["records"] % meta["n_views"]:
        raise TokenSetError(f"{out_dir}: {meta['records']} records are not whole images of {meta['n_views']} views")
    _write_json(os.path.join(out_dir, META), meta)
    return meta


# ---- dataset ---------------------------------------------------------------------------------------------------------------------------
def _open_npy(path, dtype, count):
    """memory map of one shard after checking its header and its SIZE against the record count of meta.json"""
    from numpy.lib import format as npf
    try:
        with open(path, "rb") as f:
            major, _ = npf.read_magic(f)
            shape, fortran, dt = (npf.read_array_header_1_0 if major == 1 else npf.read_array_header_2_0)(f)
            offset = f.tell()
    except (OSError, ValueError) as e:
        raise TokenSetError(f"{path}: not a readable .npy shard ({e})") from e
    if dt != dtype or fortran or len(shape) != 1:
        raise TokenSetError(f"{path}: holds {dt} {shape}, the set's records are {dtype}")
    size, want = os.path.getsize(path), offset + int(count) * dtype.itemsize
    if shape[0] != int(count) or size != want:
        raise TokenSetError(f"{path}: {shape[0]} records in {size} bytes, meta.json counts {count} records ({want} bytes)")
    if count == 0:
        return np.zeros(0, dtype=dtype)
    return np.memmap(path, dtype=dtype, mode="r", offset=offset, shape=(int(count),))


class TokenShardDataset:
    """a token set opened for random access.  Raises TokenSetError when meta.json is missing (an incomplete set), the version is
    unknown, a file's size disagrees with its count, or a code is >= codebook_size / a stored fine-cell count disagrees with its bitmap
    -- checked on the first and last record of every file at open time, on every record with verify=True."""

    def __init__(self, root, verify=False):
        self.root = str(root)
        path = os.path.join(self.root, META)
        if not os.path.exists(path):
            raise TokenSetError(f"{self.root}: no {META} -- the set is incomplete (the writer writes it last; parts need --finalize)")
        with open(path, "r", encoding="utf-8") as f:
            self.meta = json.load(f)
        if self.meta.get("version") != FORMAT_VERSION:
            raise TokenSetError(f"{self.root}: format version {self.meta.get('version')!r}, this code reads version {FORMAT_VERSION}")
        m = self.meta
        self.hw1, self.hw2, self.codebook_size, self.n_views = int(m["hw1"]), int(m["hw2"]), int(m["codebook_size"]), int(m["n_views"])
        self.dtype = record_dtype(self.hw1, self.hw2)
        self.counts = [int(f["records"]) for f in m["files"]]
        self.shards = [_open_npy(os.path.join(self.root, f["name"]), self.dtype, f["records"]) for f in m["files"]]
        self.starts = np.concatenate([[0], np.cumsum(self.counts)]).astype(np.int64)
        self.n_records = int(self.starts[-1])
        if self.n_records != int(m.get("records", self.n_records)) or self.n_views <= 0 or self.n_records % self.n_views:
            raise TokenSetError(f"{self.root}: {self.n_records} records for {self.n_views} views per image")
        self.n_images = self.n_records // self.n_views
        for i, sh in enumerate(self.shards):
            if sh.shape[0]:
                self._check(sh if verify else sh[[0, -1]], m["files"][i]["name"], int(self.starts[i]), verify)

    def _check(self, rec, name, start, full):
        if int(rec["codes"].max()) >= self.codebook_size:
            raise TokenSetError(f"{self.root}/{name}: a code >= codebook_size {self.codebook_size}")
        n = popcount_rows(rec["grain"])
        if not np.array_equal(n, rec["n_fine_cells"].astype(np.int64)):
            raise TokenSetError(f"{self.root}/{name}: a stored n_fine_cells disagrees with its bitmap")
        if full:
            want = (start + np.arange(rec.shape[0])) % self.n_views
            if not np.array_equal(rec["view"].astype(np.int64), want):
                raise TokenSetError(f"{self.root}/{name}: records are not stored image-major (record r = view r % {self.n_views})")

    def __len__(self):
        return self.n_images

    def records(self, idx) -> np.ndarray:
        """structured array of the records at the global record indices `idx` (a copy, in the order asked)"""
        idx = np.asarray(idx, dtype=np.int64).reshape(-1)
        if idx.size and (idx.min() < 0 or idx.max() >= self.n_records):
            raise IndexError(f"record index outside [0, {self.n_records})")
        out = np.empty(idx.shape[0], dtype=self.dtype)
        shard = np.searchsorted(self.starts, idx, side="right") - 1
        for s in np.unique(shard):
            sel = shard == s
            out[sel] = self.shards[int(s)][idx[sel] - self.starts[int(s)]]
        return out

    def gather(self, images, views) -> np.ndarray:
        return self.records(np.asarray(images, dtype=np.int64) * self.n_views + np.asarray(views, dtype=np.int64))

    def check_model(self, model):
        """raises TokenSetError (both fingerprints in the message) when the set was made by another first stage or for another grid"""
        want = describe_model(model)
        mine = {k: self.meta[k] for k in ("hw1", "hw2", "codebook_size", "fingerprint")}
        bad = [k for k in mine if mine[k] != want[k]]
        if bad:
            raise TokenSetError(f"{self.root} was not made for this model ({', '.join(bad)} differ): the set has hw1 {mine['hw1']}, hw2 "
                                f"{mine['hw2']}, codebook_size {mine['codebook_size']}, fingerprint {mine['fingerprint']}; the model has "
                                f"hw1 {want['hw1']}, hw2 {want['hw2']}, codebook_size {want['codebook_size']}, fingerprint "
                                f"{want['fingerprint']}")


# ---- tokeniser -------------------------------------------------------------------------------------------------------------------------
def first_stage_grid(first_stage, size, device):
    """(hw1, hw2) of a first stage: the shapes of its grain map and code map on one blank image"""
    import torch
    with torch.no_grad():
        enc = first_stage.encode(torch.zeros(1, 3, size, size, device=device))
    hw1 = int(enc[3].shape[1])
    return hw1, int(enc[2][2].shape[1]) // hw1


def tokenize_batches(first_stage, batches, writer) -> dict:
    """encode -> dvq_tokens_pack -> writer for every batch.  batches yields (views, labels, sources): `views` a list of n_views image
    tensors [b, 3, S, S] on the device (the same b images under each stored view), labels / sources integer arrays [b].  The first stage
    runs in eval mode under no_grad in the current compute dtype.  ONE synchronisation per batch: the copy of the packed records to the
    host, which carries the kernels' `bad` counts -- a non-zero count raises.  -> the tool's statistics"""
    import time

    import torch

    from . import kernels as K
    hw1, hw2, k = writer.hw1, writer.hw2, writer.header["codebook_size"]
    w, npix, ncell, nv = grain_words(hw1), (hw1 * hw2) ** 2, hw1 * hw1, writer.header["n_views"]
    first_stage.eval()
    images, tok, fine = 0, [], 0
    t0 = time.perf_counter()
    for views, labels, sources in batches:
        if len(views) != nv:
            raise ValueError(f"{len(views)} views in a batch of a set that stores {nv}")
        b, dev = int(views[0].shape[0]), views[0].device
        o1, o2, o3 = nv * b * npix * 2, nv * b * (npix * 2 + w * 4), nv * b * (npix * 2 + w * 4 + 4)
        blob = torch.empty(o3 + nv * b * 4, dtype=torch.uint8, device=dev)
        codes, bits = blob[:o1].view(torch.uint16).view(nv, b, npix), blob[o1:o2].view(torch.uint32).view(nv, b, w)
        n_fine, bad = blob[o2:o3].view(torch.int32).view(nv, b), blob[o3:].view(torch.int32).view(nv, b)
        with torch.no_grad():
            for v, x in enumerate(views):
                enc = first_stage.encode(x)
                K.tokens_pack(enc[2][2].contiguous().long(), enc[3].contiguous().long(), k, out=(codes[v], bits[v], n_fine[v], bad[v]))
        host = blob.cpu().numpy()                                         # the one synchronisation of the batch
        h_bad = host[o3:].view("<i4").reshape(nv, b)
        if h_bad.any():
            v, i = [int(a[0]) for a in np.nonzero(h_bad)]
            raise ValueError(f"image {int(sources[i])}, view {v}: {int(h_bad[v, i])} codes outside [0, {k}) or grain values other than 0 / 1")
        h_n = host[o2:o3].view("<i4").reshape(nv, b).T.reshape(-1)                                  # image-major: record = image * nv + view
        writer.append(host[:o1].view("<u2").reshape(nv, b, npix).transpose(1, 0, 2).reshape(nv * b, npix),
                      host[o1:o2].view("<u4").reshape(nv, b, w).transpose(1, 0, 2).reshape(nv * b, w), h_n,
                      np.repeat(np.asarray(labels, dtype=np.int64), nv), np.repeat(np.asarray(sources, dtype=np.int64), nv),
                      np.tile(np.arange(nv), b))
        images += b
        fine += int(h_n.sum())
        tok.append(ncell - h_n + h_n * hw2 * hw2)
    sec = time.perf_counter() - t0
    tok = np.concatenate(tok) if tok else np.zeros(0, dtype=np.int64)
    return {"images": images, "views": nv, "records": int(tok.size), "tokens_per_image": {
                "mean": float(tok.mean()) if tok.size else None, "min": int(tok.min()) if tok.size else None,
                "max": int(tok.max()) if tok.size else None},
            "fine_ratio": fine / float(tok.size * ncell) if tok.size else None, "seconds": sec, "images_per_s": images / sec if sec > 0 else None}


# ---- loader ----------------------------------------------------------------------------------------------------------------------------
def plan_epoch(n_images, n_views, batch_size, shuffle, drop_last, rng, view=None):
    """the (image indices, views) of every batch of one epoch: images in shuffled (or stored) order, one view per image drawn uniformly
    from the stored views by `rng` (view = k: always view k, nothing drawn)"""
    order = rng.permutation(n_images) if shuffle else np.arange(n_images)
    if view is not None:
        if not 0 <= int(view) < n_views:
            raise ValueError(f"view {view} of a set with {n_views} views")
        views = np.full(n_images, int(view), dtype=np.int64)
    elif n_views > 1:
        views = rng.integers(0, n_views, size=n_images)
    else:
        views = np.zeros(n_images, dtype=np.int64)
    out = [(order[i:i + batch_size].astype(np.int64), views[i:i + batch_size].astype(np.int64)) for i in range(0, n_images, batch_size)]
    if drop_last and out and len(out[-1][0]) < batch_size:
        out.pop()
    return out


class TokenBatchLoader:
    """iterates a TokenShardDataset in batches of GPU-resident stage-2 inputs, produced `prefetch` ahead of the consumer on a side stream
    (data.GpuBatchLoader's shape).  permuter: the model's DualGrainSeperatePermuter (pad / eos codes, fine-position order).  Yields
    {"tokens": the six permuter streams, "class_label": int64 [B] (when every label >= 0), "n_tokens": codes per image (host ints)}."""

    def __init__(self, dataset, batch_size, device, permuter, shuffle=False, seed=0, drop_last=True, prefetch=2, view=None):
        import torch
        self.ds, self.bs, self.device = dataset, int(batch_size), torch.device(device)
        self.shuffle, self.drop_last, self.prefetch, self.view = shuffle, drop_last, prefetch, view
        self.rng = np.random.default_rng(seed)
        if (int(permuter.hw1), int(permuter.hw2)) != (dataset.hw1, dataset.hw2):
            raise TokenSetError(f"the permuter's grid ({permuter.hw1}, {permuter.hw2}) is not the set's ({dataset.hw1}, {dataset.hw2})")
        self.order = permuter.fine_position_order
        self.codes6 = (permuter.content_pad_code, permuter.content_eos_code, permuter.coarse_position_pad_code,
                       permuter.coarse_position_eos_code, permuter.fine_position_pad_code, permuter.fine_position_eos_code)

    def __len__(self):
        n = len(self.ds)
        return n // self.bs if self.drop_last else -(-n // self.bs)

    def _batch(self, images, views):
        """gather -> one pinned buffer [labels int64 | bitmaps uint32 | codes uint16] -> ONE async copy -> ONE dvq_tokens_unpack"""
        import torch

        from . import kernels as K
        rec = self.ds.gather(images, views)
        b, hw1, hw2 = rec.shape[0], self.ds.hw1, self.ds.hw2
        n, lc, lf = batch_lengths(rec["grain"], rec["n_fine_cells"], hw1, hw2)
        w, npix = grain_words(hw1), (hw1 * hw2) ** 2
        o1, o2 = b * 8, b * 8 + b * w * 4
        host = torch.empty(o2 + b * npix * 2, dtype=torch.uint8)
        if self.device.type == "cuda":
            host = host.pin_memory()
        hb = host.numpy()
        hb[:o1].view("<i8")[:] = rec["label"]
        hb[o1:o2].view("<u4").reshape(b, w)[:] = rec["grain"]
        hb[o2:].view("<u2").reshape(b, npix)[:] = rec["codes"].reshape(b, npix)
        dev = host.to(self.device, non_blocking=True)
        tokens = K.tokens_unpack(dev[o2:].view(torch.uint16).view(b, npix), dev[o1:o2].view(torch.uint32).view(b, w), hw1, hw2,
                                 self.order, self.codes6, lc, lf, n)
        out = {"tokens": tokens, "n_tokens": (hw1 * hw1 - n + n * hw2 * hw2).tolist()}
        if (rec["label"] >= 0).all():
            out["class_label"] = dev[:o1].view(torch.int64)
        return out

    def __iter__(self):
        import torch
        batches = plan_epoch(len(self.ds), self.ds.n_views, self.bs, self.shuffle, self.drop_last, self.rng, self.view)
        q: queue.Queue = queue.Queue(maxsize=self.prefetch)
        stream = torch.cuda.Stream(self.device) if self.device.type == "cuda" else None

        def producer():
            try:
                for images, views in batches:
                    if stream is not None:
                        with torch.cuda.stream(stream):
                            b = self._batch(images, views)
                            ev = torch.cuda.Event()
                            ev.record(stream)
                    else:
                        b, ev = self._batch(images, views), None
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
                # allocated on the producer's stream, read on the consumer's: see data.GpuBatchLoader.__iter__
                for t in list(b["tokens"].values()) + [b.get("class_label")]:
                    if t is not None and t.is_cuda:
                        t.record_stream(cur)
            yield b
