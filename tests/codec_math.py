"""numpy restatement of the token codec (docs/design/27-token-codec.md): the frequency-table rule, rANS encode / decode and the
container's pack / parse, written from the specification, independent of dynamicvectorquantization_amd/codec.py and csrc/codec.hip."""
import struct
import zlib

import numpy as np

PREC = 16
M = 1 << PREC
L = 1 << 31
MASK32 = (1 << 32) - 1


# ---------------------------------------------------------------------------------------------
# the allowed set and the table
# ---------------------------------------------------------------------------------------------
def allowed_mask(x, forbid_idx=(), forbid_from=None, forbid_codes=(), keep_code=-1, late_forbid_code=-1, pad_code=0, finished=False):
    """A of one row x [V]: a finished row keeps pad_code only; a live row loses the listed columns, every column >= forbid_from and the
    forbid_codes, gets keep_code back, loses late_forbid_code -- and every column whose logit is not finite"""
    v = len(x)
    if finished:
        a = np.zeros(v, dtype=bool)
        a[pad_code] = True
        return a
    masked = np.zeros(v, dtype=bool)
    for c in forbid_idx:
        if 0 <= c < v:
            masked[c] = True
    if forbid_from is not None and 0 <= forbid_from < v:
        masked[forbid_from:] = True
    for c in forbid_codes:
        if 0 <= c < v:
            masked[c] = True
    if 0 <= keep_code < v:
        masked[keep_code] = False
    if 0 <= late_forbid_code < v:
        masked[late_forbid_code] = True
    return ~masked & np.isfinite(np.asarray(x, dtype=np.float64))


def _ordered_sum(e):
    """fp32 sum of e [V] in the specified order: lane l of 64 adds columns l, l + 64, ... in ascending order, then the xor tree"""
    part = np.zeros(64, dtype=np.float32)
    for i in range(0, len(e), 64):
        chunk = e[i:i + 64]
        part[:len(chunk)] = part[:len(chunk)] + chunk
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        part = (part + part[lanes ^ o]).astype(np.float32)
    return np.float32(part[0])


def table(x, allowed):
    """f uint32 [V] of one row of logits x (fp32 values) over the allowed set: sum f = M, f >= 1 on A, 0 elsewhere"""
    x = np.asarray(x, dtype=np.float32)
    a = np.asarray(allowed, dtype=bool)
    n = int(a.sum())
    f = np.zeros(len(x), dtype=np.int64)
    if n == 0:
        return f.astype(np.uint32)
    cols = np.nonzero(a)[0]
    m = np.float32(x[cols].max())
    amax = int(cols[np.argmax(x[cols] == m)])                # lowest-index arg-max of A
    if n == 1:
        f[amax] = M
        return f.astype(np.uint32)
    with np.errstate(under="ignore"):
        e = np.where(a, np.exp((np.where(a, x, m) - m).astype(np.float32)).astype(np.float32), np.float32(0)).astype(np.float32)
    s = _ordered_sum(e)
    q = ((e / s).astype(np.float32) * np.float32(M - n)).astype(np.float32)
    f[a] = 1 + np.floor(q[a]).astype(np.int64)
    f[amax] += M - int(f.sum())
    return f.astype(np.uint32)


def cumulative(f):
    """exclusive prefix sums in column order"""
    f = np.asarray(f, dtype=np.int64)
    return np.cumsum(f) - f


# ---------------------------------------------------------------------------------------------
# rANS: 64-bit state, lower bound 2^31, 32-bit words, 16-bit frequencies
# ---------------------------------------------------------------------------------------------
def rans_encode(records):
    """records: sequence of (cum, f) in FORWARD order (None or f == 0: the step codes nothing) -> uint32 words in the order the decoder
    reads them: the final state's low and high half, then the renormalisation words, last emitted first"""
    x = L
    out = []                                                  # in emission order; the stream is its reverse
    for r in reversed(list(records)):
        if r is None:
            continue
        cum, f = int(r[0]), int(r[1])
        if f == 0:
            continue
        assert 0 < f < M and 0 <= cum and cum + f <= M
        if x >= (((L >> PREC) << 32) * f):
            out.append(x & MASK32)
            x >>= 32
        x = ((x // f) << PREC) + (x % f) + cum
        assert L <= x < (L << 32)
    out.append(x >> 32)
    out.append(x & MASK32)
    return np.asarray(out[::-1], dtype=np.uint32)


def unpack_records(packed):
    """the device's records (cum | f << 16, 0 = nothing coded) -> list for rans_encode"""
    p = np.asarray(packed).astype(np.int64) & MASK32
    return [None if (v >> 16) == 0 else (int(v & 0xFFFF), int(v >> 16)) for v in p.tolist()]


class RansDecoder:
    def __init__(self, words):
        self.words = [int(w) for w in np.asarray(words, dtype=np.uint32)]
        assert len(self.words) >= 2
        self.x = self.words[0] | (self.words[1] << 32)
        self.cursor = 2
        self.underrun = False

    def symbol(self, f):
        """the column under the state for the table f [V]; advances the state"""
        f = np.asarray(f, dtype=np.int64)
        cum = cumulative(f)
        slot = self.x & (M - 1)
        c = int(np.searchsorted(cum + f, slot, side="right"))
        assert cum[c] <= slot < cum[c] + f[c]
        self.x = int(f[c]) * (self.x >> PREC) + slot - int(cum[c])
        if self.x < L:
            w = 0
            if self.cursor < len(self.words):
                w = self.words[self.cursor]
                self.cursor += 1
            else:
                self.underrun = True
            self.x = (self.x << 32) | w
        return c


def ideal_bits(records):
    return float(sum(np.log2(M / r[1]) for r in records if r is not None and r[1] > 0))


# ---------------------------------------------------------------------------------------------
# container (little-endian; the layout table of the design note)
# ---------------------------------------------------------------------------------------------
class ContainerError(Exception):
    pass


def pack(groups, group_size, fingerprint, dtype_code, step_code, coarse_hw, fine_hw, with_labels):
    n_images = sum(len(w) for _, w in groups)
    head = b"DQTC" + struct.pack("<HBBIIBBHHH", 1, dtype_code, step_code, group_size, n_images, int(with_labels), 0, coarse_hw, fine_hw, 0)
    head += bytes(fingerprint) + struct.pack("<I", 0)
    out = head + struct.pack("<I", zlib.crc32(head))
    for labels, words in groups:
        body = struct.pack("<I", len(words))
        if with_labels:
            body += b"".join(struct.pack("<i", int(v)) for v in labels)
        body += b"".join(struct.pack("<I", len(w)) for w in words)
        body += b"".join(struct.pack("<I", int(v)) for w in words for v in w)
        out += body + struct.pack("<I", zlib.crc32(body))
    return out


def parse(blob):
    def take(fmt, off):
        size = struct.calcsize(fmt)
        if off + size > len(blob):
            raise ContainerError("truncated")
        return struct.unpack_from(fmt, blob, off), off + size

    (magic,), off = take("<4s", 0)
    if magic != b"DQTC":
        raise ContainerError("magic")
    (version, dtype_code, step_code, group_size, n_images, with_labels, _, coarse_hw, fine_hw, _), off = take("<HBBIIBBHHH", off)
    (fingerprint, _), off = take("<8sI", off)
    (crc,), off = take("<I", off)
    if version != 1 or crc != zlib.crc32(blob[:36]):
        raise ContainerError("header")
    groups, left = [], n_images
    while left > 0:
        start = off
        (n,), off = take("<I", off)
        if n != min(group_size, left):
            raise ContainerError("group size")
        labels = None
        if with_labels:
            labels, off = take(f"<{n}i", off)
        counts, off = take(f"<{n}I", off)
        words = []
        for k in counts:
            if k < 2:
                raise ContainerError("count")
            w, off = take(f"<{k}I", off)
            words.append(np.asarray(w, dtype=np.uint32))
        end = off
        (crc,), off = take("<I", off)
        if crc != zlib.crc32(blob[start:end]):
            raise ContainerError("crc")
        groups.append((None if labels is None else np.asarray(labels, dtype=np.int32), words))
        left -= n
    if off != len(blob):
        raise ContainerError("trailing bytes")
    header = dict(dtype_code=dtype_code, step_code=step_code, group_size=group_size, n_images=n_images, with_labels=bool(with_labels),
                  coarse_hw=coarse_hw, fine_hw=fine_hw, fingerprint=fingerprint)
    return header, groups
