"""numpy restatement of the device JPEG decode (include/dvq_hip.h: dvq_jpeg_entropy_decode, dvq_jpeg_batch_decode) and the case matrix its
tests share.  No GPU, no library: a slow bit-at-a-time Huffman decoder in Python, then libjpeg-turbo's default arithmetic written out
with numpy integers -- the "islow" inverse DCT (jidctint.c), fancy chroma upsampling (jdsample.c) and the fixed-point colour conversion
(jdcolor.c).  tests/test_jpeg_cpu.py holds it against PIL, pixel for pixel; tests/test_gpu_jpeg.py holds the kernels against it."""
import io

import numpy as np

NATURAL = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                    35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55,
                    62, 63])


# ---- the case matrix: the smallest shapes at which each piece can go wrong ---------------------------------------------------------
# (name, w, h, mode, save options).  subsampling: 0 = 4:4:4, 1 = 4:2:2, 2 = 4:2:0
CASES = [
    ("1x1", 1, 1, "RGB", dict(quality=92, subsampling=2)),
    ("8x8", 8, 8, "RGB", dict(quality=92, subsampling=2)),
    ("16x16", 16, 16, "RGB", dict(quality=92, subsampling=2)),
    ("17x9_q30_opt", 17, 9, "RGB", dict(quality=30, subsampling=2, optimize=True)),
    ("45x37_420", 45, 37, "RGB", dict(quality=85, subsampling=2)),
    ("33x50_422", 33, 50, "RGB", dict(quality=75, subsampling=1)),
    ("40x24_444", 40, 24, "RGB", dict(quality=90, subsampling=0)),
    ("31x29_grey", 31, 29, "L", dict(quality=80)),
    ("64x48_rst3", 64, 48, "RGB", dict(quality=95, subsampling=2, restart_marker_blocks=3)),
    ("20x20_rst1", 20, 20, "RGB", dict(quality=92, subsampling=2, restart_marker_blocks=1)),
    ("50x50_q100", 50, 50, "RGB", dict(quality=100, subsampling=2)),
    ("9x17_422", 9, 17, "RGB", dict(quality=92, subsampling=1)),
    ("23x8_420", 23, 8, "RGB", dict(quality=92, subsampling=2)),
    # chroma planes of 1 and 2 columns: libjpeg replicates there instead of filtering
    ("3x5_420", 3, 5, "RGB", dict(quality=92, subsampling=2)),
    ("4x4_422", 4, 4, "RGB", dict(quality=92, subsampling=1)),
    ("5x3_420", 5, 3, "RGB", dict(quality=92, subsampling=2)),
    ("500x375_420", 500, 375, "RGB", dict(quality=90, subsampling=2)),
]


def test_image(w, h, mode, seed):
    """smooth gradients + edges + noise: every coefficient position gets used, and quality 100 reaches the clamps"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    ch = []
    for c in range(3):
        base = 127.5 + 110 * np.sin(xx / (3.0 + c) + c) * np.cos(yy / (4.0 + 2 * c))
        base = base + 90 * (((xx // 5 + yy // 7 + c) % 2) - 0.5)
        base = base + rng.normal(0, 25, size=(h, w))
        ch.append(np.clip(base, 0, 255))
    a = np.stack(ch, axis=-1).astype(np.uint8)
    return a if mode == "RGB" else a[..., 0].copy()


def encode(w, h, mode, opts, seed=0):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(test_image(w, h, mode, seed), mode).save(buf, "JPEG", **opts)
    return buf.getvalue()


_case_cache = {}


def case_bytes(name):
    """the JPEG bytes of a case, written once per process"""
    if name not in _case_cache:
        i = [c[0] for c in CASES].index(name)
        _, w, h, mode, opts = CASES[i]
        _case_cache[name] = encode(w, h, mode, opts, seed=i)
    return _case_cache[name]


def pil_rgb(data):
    from PIL import Image
    with Image.open(io.BytesIO(data)) as im:
        return np.asarray(im.convert("RGB"), dtype=np.uint8)


# ---- slow entropy decoder ----------------------------------------------------------------------------------------------------------
def parse(data):
    """markers up to the first SOS of a baseline JPEG -> dict(w, h, comps [(id, h, v, tq)], q {tq: int [64] natural}, huff {(tc, th):
    {(length, code): symbol}}, ri, scan [(td, ta)], scan_off)"""
    assert data[:2] == b"\xff\xd8"
    pos, out = 2, dict(q={}, huff={}, ri=0)
    while True:
        assert data[pos] == 0xFF
        while data[pos] == 0xFF:
            pos += 1
        m = data[pos]
        pos += 1
        if m == 0x01 or 0xD0 <= m <= 0xD8:
            continue
        n = (data[pos] << 8) | data[pos + 1]
        seg = data[pos + 2:pos + n]
        if m in (0xC0, 0xC1):
            assert seg[0] == 8
            out["h"], out["w"] = (seg[1] << 8) | seg[2], (seg[3] << 8) | seg[4]
            out["comps"] = [(seg[6 + 3 * i], seg[7 + 3 * i] >> 4, seg[7 + 3 * i] & 15, seg[8 + 3 * i]) for i in range(seg[5])]
        elif m == 0xDB:
            o = 0
            while o < len(seg):
                pq, tq = seg[o] >> 4, seg[o] & 15
                o += 1
                t = np.zeros(64, dtype=np.int64)
                for k in range(64):
                    t[NATURAL[k]] = ((seg[o + 2 * k] << 8) | seg[o + 2 * k + 1]) if pq else seg[o + k]
                o += 64 * (pq + 1)
                out["q"][tq] = t
        elif m == 0xC4:
            o = 0
            while o < len(seg):
                tc, th = seg[o] >> 4, seg[o] & 15
                bits = list(seg[o + 1:o + 17])
                o += 17
                table, code = {}, 0
                for length in range(1, 17):
                    for _ in range(bits[length - 1]):
                        table[(length, code)] = seg[o]
                        o += 1
                        code += 1
                    code <<= 1
                out["huff"][(tc, th)] = table
        elif m == 0xDD:
            out["ri"] = (seg[0] << 8) | seg[1]
        elif m == 0xDA:
            ns = seg[0]
            assert ns == len(out["comps"])
            out["scan"] = [(seg[2 + 2 * i] >> 4, seg[2 + 2 * i] & 15) for i in range(ns)]
            out["scan_off"] = pos + n
            return out
        else:
            assert m not in (0xC2, 0xC9, 0xCA), "not a baseline JPEG"
        pos += n


class _BitReader:
    def __init__(self, data, pos):
        self.d, self.p, self.acc, self.n = data, pos, 0, 0

    def bit(self):
        if self.n == 0:
            b = self.d[self.p]
            self.p += 1
            if b == 0xFF:
                assert self.d[self.p] == 0, "marker inside entropy data"
                self.p += 1
            self.acc, self.n = b, 8
        self.n -= 1
        return (self.acc >> self.n) & 1

    def bits(self, k):
        v = 0
        for _ in range(k):
            v = (v << 1) | self.bit()
        return v

    def symbol(self, table):
        code = 0
        for length in range(1, 17):
            code = (code << 1) | self.bit()
            if (length, code) in table:
                return table[(length, code)]
        raise AssertionError("no such Huffman code")

    def restart(self, k):
        self.n = 0
        assert self.d[self.p] == 0xFF and self.d[self.p + 1] == 0xD0 + (k & 7), "restart marker expected"
        self.p += 2


def _extend(v, s):
    return v - (1 << s) + 1 if v < (1 << (s - 1)) else v


def geometry(hdr):
    """-> (ncomp, hs, vs, mcux, mcuy, [(block rows, block cols) per component])"""
    comps = hdr["comps"]
    nc = len(comps)
    hs, vs = (comps[0][1], comps[0][2]) if nc == 3 else (1, 1)
    mcux, mcuy = -(-hdr["w"] // (8 * hs)), -(-hdr["h"] // (8 * vs))
    grids = [(mcuy * vs, mcux * hs)] + [(mcuy, mcux)] * (nc - 1)
    return nc, hs, vs, mcux, mcuy, grids


def entropy_decode(data):
    """-> (coef: list per component of int16 [block_rows, block_cols, 64] in natural order, not dequantised; qtab uint16 [ncomp, 64])"""
    hdr = parse(data)
    nc, hs, vs, mcux, mcuy, grids = geometry(hdr)
    coef = [np.zeros((r, c, 64), dtype=np.int16) for r, c in grids]
    samp = [(hs, vs)] + [(1, 1)] * (nc - 1)
    br = _BitReader(data, hdr["scan_off"])
    pred, mcu, rst = [0] * nc, 0, 0
    for my in range(mcuy):
        for mx in range(mcux):
            if hdr["ri"] and mcu and mcu % hdr["ri"] == 0:
                br.restart(rst)
                rst += 1
                pred = [0] * nc
            for c in range(nc):
                dc, ac = hdr["huff"][(0, hdr["scan"][c][0])], hdr["huff"][(1, hdr["scan"][c][1])]
                for v in range(samp[c][1]):
                    for h in range(samp[c][0]):
                        blk = coef[c][my * samp[c][1] + v, mx * samp[c][0] + h]
                        s = br.symbol(dc)
                        if s:
                            pred[c] += _extend(br.bits(s), s)
                        blk[0] = pred[c]
                        k = 1
                        while k < 64:
                            rs = br.symbol(ac)
                            r, s = rs >> 4, rs & 15
                            if s == 0:
                                if r != 15:
                                    break
                                k += 16
                                continue
                            k += r
                            blk[NATURAL[k]] = _extend(br.bits(s), s)
                            k += 1
            mcu += 1
    qtab = np.stack([hdr["q"][comp[3]] for comp in hdr["comps"]]).astype(np.uint16)
    return coef, qtab


# ---- stage (a): dequantise, inverse DCT, + 128, clamp ------------------------------------------------------------------------------
def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def _idct8(c, shift):
    """c: int64 [..., 8] -> [..., 8]: one pass of jpeg_idct_islow along the last axis"""
    c = [c[..., i] for i in range(8)]
    z1 = (c[2] + c[6]) * 4433
    t2 = z1 - c[6] * 15137
    t3 = z1 + c[2] * 6270
    t0 = (c[0] + c[4]) << 13
    t1 = (c[0] - c[4]) << 13
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    a0, a1, a2, a3 = c[7], c[5], c[3], c[1]
    z1, z2, z3, z4 = a0 + a3, a1 + a2, a0 + a2, a1 + a3
    z5 = (z3 + z4) * 9633
    a0, a1, a2, a3 = a0 * 2446, a1 * 16819, a2 * 25172, a3 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    a0, a1, a2, a3 = a0 + z1 + z3, a1 + z2 + z4, a2 + z2 + z3, a3 + z1 + z4
    out = [t10 + a3, t11 + a2, t12 + a1, t13 + a0, t13 - a0, t12 - a1, t11 - a2, t10 - a3]
    return np.stack([_descale(o, shift) for o in out], axis=-1)


def idct_planes(coef, qtab):
    """-> list per component of uint8 [block_rows * 8, block_cols * 8] (the padded planes)"""
    planes = []
    for c, cf in enumerate(coef):
        rows, cols = cf.shape[:2]
        x = cf.astype(np.int64) * qtab[c].astype(np.int64)
        x = x.reshape(rows, cols, 8, 8)
        ws = np.swapaxes(_idct8(np.swapaxes(x, -1, -2), 11), -1, -2)       # column pass: along the row index
        px = np.clip(_idct8(ws, 18) + 128, 0, 255).astype(np.uint8)        # row pass
        planes.append(px.transpose(0, 2, 1, 3).reshape(rows * 8, cols * 8))
    return planes


# ---- stage (b): fancy upsampling and colour ----------------------------------------------------------------------------------------
def _h2v1(s):
    """s int64 [rows, cw] -> [rows, 2 * cw] (h2v1_fancy_upsample; planes of 1 or 2 columns are replicated instead)"""
    cw = s.shape[1]
    if cw <= 2:
        return np.repeat(s, 2, axis=1)
    left = np.concatenate([s[:, :1], s[:, :-1]], axis=1)
    right = np.concatenate([s[:, 1:], s[:, -1:]], axis=1)
    out = np.empty((s.shape[0], 2 * cw), dtype=np.int64)
    out[:, 0::2] = (3 * s + left + 1) >> 2
    out[:, 1::2] = (3 * s + right + 2) >> 2
    out[:, 0], out[:, -1] = s[:, 0], s[:, -1]
    return out


def _h2v2(s):
    """s int64 [ch, cw] -> [2 * ch, 2 * cw] (h2v2_fancy_upsample; planes of 1 or 2 columns are replicated instead)"""
    ch, cw = s.shape
    if cw <= 2:
        return np.repeat(np.repeat(s, 2, axis=0), 2, axis=1)
    up = np.concatenate([s[:1], s[:-1]], axis=0)
    down = np.concatenate([s[1:], s[-1:]], axis=0)
    out = np.empty((2 * ch, 2 * cw), dtype=np.int64)
    for v, near in ((0, up), (1, down)):
        cs = 3 * s + near
        left = np.concatenate([cs[:, :1], cs[:, :-1]], axis=1)
        right = np.concatenate([cs[:, 1:], cs[:, -1:]], axis=1)
        row = np.empty((ch, 2 * cw), dtype=np.int64)
        row[:, 0::2] = (3 * cs + left + 8) >> 4
        row[:, 1::2] = (3 * cs + right + 7) >> 4
        row[:, 0], row[:, -1] = (4 * cs[:, 0] + 8) >> 4, (4 * cs[:, -1] + 7) >> 4
        out[v::2] = row
    return out


def _fix(v):
    return int(v * 65536 + 0.5)


def planes_to_rgb(planes, w, h, hs, vs):
    """-> uint8 [h, w, 3]"""
    y = planes[0][:h, :w].astype(np.int64)
    if len(planes) == 1:
        return np.repeat(y[..., None], 3, axis=-1).astype(np.uint8)
    cw, ch = -(-w // hs), -(-h // vs)
    chroma = []
    for p in planes[1:]:
        s = p[:ch, :cw].astype(np.int64)            # the real plane: the padding of the block grid is never read
        if (hs, vs) == (2, 1):
            s = _h2v1(s)
        elif (hs, vs) == (2, 2):
            s = _h2v2(s)
        else:
            assert (hs, vs) == (1, 1)
        chroma.append(s[:h, :w] - 128)
    cb, cr = chroma
    r = y + ((_fix(1.402) * cr + 32768) >> 16)
    g = y + ((-_fix(0.34414) * cb + 32768 - _fix(0.71414) * cr) >> 16)
    b = y + ((_fix(1.772) * cb + 32768) >> 16)
    return np.clip(np.stack([r, g, b], axis=-1), 0, 255).astype(np.uint8)


def decode(data):
    """the whole restatement: JPEG bytes -> uint8 [h, w, 3]"""
    hdr = parse(data)
    nc, hs, vs, mcux, mcuy, grids = geometry(hdr)
    coef, qtab = entropy_decode(data)
    return planes_to_rgb(idct_planes(coef, qtab), hdr["w"], hdr["h"], hs, vs)


def coef_count(data):
    return sum(r * c * 64 for r, c in geometry(parse(data))[5])
