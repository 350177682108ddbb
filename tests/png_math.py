"""Helpers of the PNG tests (not collected): a small PNG writer that applies a CHOSEN filter type per row (PIL cannot be told which
filter to use, so the tests write their own files and let PIL decode them: that is the oracle), and a numpy restatement of the
un-filtering that csrc/png.hip does on the device (docs/design/29-device-png.md)."""
import io
import struct
import zlib

import numpy as np

SIGNATURE = b"\x89PNG\r\n\x1a\n"
COLOUR_TYPE = {1: 0, 2: 4, 3: 2, 4: 6}        # bytes per pixel -> PNG colour type (8 bits per sample)


def chunk(kind, body=b""):
    return struct.pack(">I", len(body)) + kind + body + struct.pack(">I", zlib.crc32(kind + body))


def _paeth(a, b, c):
    """the PNG specification's predictor on int arrays"""
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    return np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))


def _predict(ft, a, b, c):
    if ft == 0:
        return np.zeros_like(a)
    if ft == 1:
        return a
    if ft == 2:
        return b
    if ft == 3:
        return (a + b) >> 1
    return _paeth(a, b, c)


def filter_rows(pix, filters):
    """pix uint8 [h, w, bpp], one filter type (0..4) per row -> the filtered scanlines uint8 [h * (1 + w * bpp)]"""
    h, w, bpp = pix.shape
    raw = pix.reshape(h, w * bpp).astype(np.int64)
    left = np.concatenate([np.zeros((h, bpp), np.int64), raw[:, :-bpp]], axis=1) if w > 0 else raw
    up = np.concatenate([np.zeros((1, w * bpp), np.int64), raw[:-1]], axis=0)
    upleft = np.concatenate([np.zeros((h, bpp), np.int64), up[:, :-bpp]], axis=1)
    out = np.empty((h, 1 + w * bpp), dtype=np.uint8)
    for y in range(h):
        ft = int(filters[y])
        out[y, 0] = ft
        out[y, 1:] = ((raw[y] - _predict(ft, left[y], up[y], upleft[y])) & 255).astype(np.uint8)
    return out.reshape(-1)


def write_png(pix, filters, idat_chunks=1, level=6, extra=(), colour_type=None, depth=8, interlace=0):
    """pix uint8 [h, w, bpp] (bpp 1 grey, 2 grey + alpha, 3 RGB, 4 RGBA), filters: one type per row -> the file's bytes.
    idat_chunks: the deflate stream is split into that many IDAT chunks; extra: chunks placed between IHDR and the first IDAT"""
    h, w, bpp = pix.shape
    z = zlib.compress(filter_rows(pix, filters).tobytes(), level)
    return assemble(w, h, COLOUR_TYPE[bpp] if colour_type is None else colour_type, z, idat_chunks, extra, depth, interlace)


def assemble(w, h, colour_type, z, idat_chunks=1, extra=(), depth=8, interlace=0):
    """a file around an already deflated stream `z`"""
    cuts = [len(z) * i // idat_chunks for i in range(idat_chunks + 1)]
    body = b"".join(chunk(b"IDAT", z[cuts[i]:cuts[i + 1]]) for i in range(idat_chunks))
    return SIGNATURE + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, depth, colour_type, 0, 0, interlace)) + b"".join(extra) + body + \
        chunk(b"IEND")


def unfilter(scan, w, h, bpp):
    """the device stage restated: filtered scanlines uint8 [h * (1 + w * bpp)] -> pixels uint8 [h, w, bpp].  Per byte lane: a = left, b =
    above, c = above left, zero outside the image; result = (filtered + predictor) & 255"""
    rows = np.asarray(scan, dtype=np.uint8).reshape(h, 1 + w * bpp)
    out = np.zeros((h + 1, w + 1, bpp), dtype=np.int64)          # a zero row above and a zero column to the left
    for y in range(h):
        ft = int(rows[y, 0])
        assert ft <= 4
        f = rows[y, 1:].reshape(w, bpp).astype(np.int64)
        b, c = out[y, 1:], out[y, :-1]
        if ft in (0, 2):
            out[y + 1, 1:] = (f + _predict(ft, b, b, c)) & 255
            continue
        for x in range(w):
            out[y + 1, x + 1] = (f[x] + _predict(ft, out[y + 1, x], b[x], c[x])) & 255
    return out[1:, 1:].astype(np.uint8)


def to_rgb(pix):
    """what the device writes for decoded pixels [h, w, bpp]: grey to all three channels, alpha dropped"""
    bpp = pix.shape[2]
    return np.ascontiguousarray(np.repeat(pix[..., :1], 3, axis=2) if bpp < 3 else pix[..., :3])


def pil_rgb(data):
    """the oracle: PIL's decode, converted to RGB as data.decode_rgb does"""
    from PIL import Image
    with Image.open(io.BytesIO(data)) as im:
        if im.mode != "RGB":
            im = im.convert("RGB")
        return np.asarray(im, dtype=np.uint8)


def picture(w, h, bpp, seed):
    """smooth shading + edges + noise, every byte lane different"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    ch = []
    for c in range(bpp):
        base = 127.5 + 100 * np.sin(xx / (3.0 + c) + c) * np.cos(yy / (4.0 + 2 * c)) + 80 * (((xx // 5 + yy // 7 + c) % 2) - 0.5)
        ch.append(np.clip(base + rng.normal(0, 30, size=(h, w)), 0, 255))
    return np.stack(ch, axis=-1).astype(np.uint8)


def cases():
    """the case matrix: (name, pix uint8 [h, w, bpp], filters [h], idat_chunks).  Widths 1, 2, 3, 5, 63, 64, 65, 257 (odd pitch,
    narrower than the lane skew, just past a wave), heights 1, 2, 63, 64, 65, 129 (band edges, three bands), bpp 1..4, random filters, and
    the directed cases.  Every image is under 260 x 130."""
    rng = np.random.default_rng(2024)
    out = []
    widths, heights = [1, 2, 3, 5, 63, 64, 65, 257], [1, 2, 63, 64, 65, 129]
    n = 0
    for i, w in enumerate(widths):                       # every width and every height, every bpp with each of them at least once
        for j, h in enumerate(heights):
            if (i + j) % 2 and not (w == 257 and h == 129):
                continue
            bpp = 1 + n % 4
            n += 1
            out.append((f"{w}x{h}x{bpp}", picture(w, h, bpp, 100 + n), rng.integers(0, 5, size=h), 1))
    for bpp in (1, 2, 3, 4):
        out.append((f"257x129x{bpp}-bands", picture(257, 129, bpp, 300 + bpp), rng.integers(0, 5, size=129), 1))
    for ft in range(5):                                  # one filter on every row: row 0 and column 0 meet each of them
        out.append((f"all-{ft}", picture(37, 70, 3, 400 + ft), np.full(70, ft), 1))
        out.append((f"all-{ft}-rgba", picture(66, 5, 4, 410 + ft), np.full(5, ft), 1))
    # Paeth ties.  pa == pb needs a == b or pc == 0; the ties that decide a pixel are pa == pc (a over c: c = 100, b = 50, a = 200) and
    # pb == pc (b over c: c = 100, a = 50, b = 200): a picture of five levels 50 apart has plenty of each
    ties = (rng.integers(0, 5, size=(67, 45, 3)) * 50).astype(np.uint8)
    out.append(("paeth-ties", ties, np.full(67, 4), 1))
    sym = np.zeros((6, 6, 1), np.uint8)
    sym[:] = [[[10], [20], [10], [20], [30], [30]]] * 6   # a == b != c and b == c != a along the rows
    sym[1::2] += 10
    out.append(("paeth-ties-directed", sym, np.full(6, 4), 1))
    bright = (200 + rng.integers(0, 56, size=(66, 70, 4))).astype(np.uint8)
    out.append(("average-carry", bright, np.full(66, 3), 1))          # a + b >= 256 everywhere
    ext = (rng.integers(0, 2, size=(65, 64, 3)) * 255).astype(np.uint8)
    out.append(("wrap-0-255", ext, rng.integers(0, 5, size=65), 1))
    out.append(("idat-3-chunks", picture(130, 90, 3, 500), rng.integers(0, 5, size=90), 3))
    return out
