"""The token codec without a GPU (docs/design/27-token-codec.md): the table rule's invariants on adversarial rows, rANS round trips
and the overhead bound in the numpy restatement (tests/codec_math.py), and the container of dynamicvectorquantization_amd.codec --
its bytes against the restatement's, and every way a blob is rejected before anything would be decoded."""
import struct
import zlib

import numpy as np
import pytest

import codec_math as cm

M = cm.M


def _check_table(f, allowed):
    f = f.astype(np.int64)
    assert int(f.sum()) == M
    assert (f[allowed] >= 1).all()
    assert (f[~allowed] == 0).all()


def _adversarial_rows():
    rng = np.random.default_rng(5)
    rows = []
    for n in (2, 1027, 2048):                                            # uniform rows: every floor loses the most it can
        rows.append((f"uniform{n}", np.full(n, 0.37, dtype=np.float32), np.ones(n, dtype=bool)))
    for sign in (80.0, -80.0):                                           # one-hot: every other exp underflows / the hot one does
        x = np.zeros(1027, dtype=np.float32)
        x[413] = sign
        rows.append((f"onehot{sign:+.0f}", x, np.ones(1027, dtype=bool)))
    x = rng.normal(0, 3, 259).astype(np.float32)
    x[[0, 17, 258]] = -np.inf                                            # -inf columns leave the allowed set
    rows.append(("neginf", x, cm.allowed_mask(x)))
    x = rng.normal(0, 2, 515).astype(np.float32)
    x[[7, 300, 514]] = x.max() + 1.5                                     # exact ties at the maximum
    rows.append(("ties", x, np.ones(515, dtype=bool)))
    x = rng.normal(0, 2, 67).astype(np.float32)
    a = np.zeros(67, dtype=bool)
    a[41] = True                                                         # n = 1
    rows.append(("single", x, a))
    x = rng.normal(0, 6, 2048).astype(np.float32)
    rows.append(("random2048", x, rng.random(2048) < 0.7))
    return rows


@pytest.mark.parametrize("name,x,allowed", _adversarial_rows(), ids=[r[0] for r in _adversarial_rows()])
def test_table_invariants(name, x, allowed):
    f = cm.table(x, allowed)
    _check_table(f, allowed)
    if name.startswith("uniform"):
        n = len(x)
        assert int(f.max()) - int(f.min()) <= n                          # the remainder (at most n) lands on column 0
        assert int(np.argmax(f)) == 0
    if name == "ties":
        g = f.astype(np.int64)
        assert g[300] == g[514] and g[7] >= g[300]                       # the remainder goes to the LOWEST arg-max
    if name == "single":
        assert int(f[41]) == M
    if name == "neginf":
        assert (f[[0, 17, 258]] == 0).all()


def test_allowed_mask_rule_order():
    x = np.zeros(12, dtype=np.float32)
    a = cm.allowed_mask(x, forbid_idx=[1, 2, 9], forbid_from=8, forbid_codes=(3,), keep_code=9, late_forbid_code=2, pad_code=8)
    assert np.nonzero(a)[0].tolist() == [0, 4, 5, 6, 7, 9]               # keep_code 9 comes back although listed and >= forbid_from
    a = cm.allowed_mask(x, forbid_idx=[1], keep_code=5, late_forbid_code=5, pad_code=3)
    assert not a[5]                                                      # late_forbid_code wins over keep_code
    a = cm.allowed_mask(x, forbid_idx=[1], pad_code=3, finished=True)
    assert np.nonzero(a)[0].tolist() == [3]


def _random_tables(rng, count, v):
    tabs = []
    for _ in range(count):
        a = rng.random(v) < rng.choice([0.05, 0.5, 1.0])
        if a.sum() < 2:
            a[:2] = True
        tabs.append(cm.table(rng.normal(0, rng.choice([0.5, 3, 12]), v).astype(np.float32), a))
    return tabs


def _round_trip(tabs, syms):
    recs = [(int(cm.cumulative(t)[s]), int(t[s])) for t, s in zip(tabs, syms)]
    words = cm.rans_encode(recs)
    dec = cm.RansDecoder(words)
    got = [dec.symbol(t) for t in tabs]
    assert got == list(syms)
    assert dec.x == cm.L and dec.cursor == len(words) and not dec.underrun
    return words, recs


@pytest.mark.parametrize("length", [0, 1, 3000])
def test_rans_round_trip_and_overhead(length):
    rng = np.random.default_rng(100 + length)
    pool = _random_tables(rng, 24, 515)
    tabs = [pool[i] for i in rng.integers(0, len(pool), length)]
    syms = [int(rng.choice(np.nonzero(t)[0], p=t[t > 0] / M)) if rng.random() < 0.8 else int(rng.choice(np.nonzero(t)[0])) for t in tabs]
    words, recs = _round_trip(tabs, syms)
    assert len(words) <= length + 2                                      # a symbol emits at most one word
    # 32 x renormalisation words + 64 <= ideal + 100: 64 bits of flushed state (the stream's first two words), a partial word, and at
    # most log2(1 + 2^-15) per symbol.  len(words) counts the two state words, so the left side is 32 x len(words)
    assert 32 * (len(words) - 2) + 64 <= cm.ideal_bits(recs) + 100


def test_rans_cheap_symbols():
    """many symbols with f = M - n + 1 (log2(M / f) ~ 1e-4 bits each): a 16-bit state would spend up to a bit on each"""
    n, length = 7, 3000
    f = np.ones(n, dtype=np.uint32)
    f[3] = M - n + 1
    assert int(f.sum()) == M
    rng = np.random.default_rng(9)
    syms = [3 if rng.random() < 0.999 else int(rng.integers(0, n)) for _ in range(length)]
    words, recs = _round_trip([f] * length, syms)
    bits = cm.ideal_bits(recs)
    assert 32 * (len(words) - 2) + 64 <= bits + 100
    assert 32 * len(words) < 0.2 * length                                # far below one bit per symbol


def test_rans_skips_and_underrun():
    f = cm.table(np.linspace(-2, 2, 19).astype(np.float32), np.ones(19, dtype=bool))
    cum = cm.cumulative(f)
    syms = [4, 18, 0, 7] * 40
    recs = []
    for s in syms:
        recs += [(int(cum[s]), int(f[s])), None]                         # every other step codes nothing
    words = cm.rans_encode(recs)
    assert np.array_equal(words, cm.rans_encode([r for r in recs if r is not None]))
    dec = cm.RansDecoder(words[:-1])                                     # one word short: zeros come in, the flag goes up
    for _ in syms:
        dec.symbol(f)
    assert dec.underrun


def test_labels_are_checked_on_the_host():
    """class labels index embedding tables on the device: anything outside [0, n_classes) raises before it gets there"""
    from dynamicvectorquantization_amd import codec
    codec.check_labels(None, None)
    codec.check_labels(np.asarray([0, 9, 3], dtype=np.int32), 10)
    for bad in ([0, 10], [-1, 2], [2 ** 31 - 1], [-2 ** 31]):
        with pytest.raises(codec.CodecError, match="class label"):
            codec.check_labels(np.asarray(bad, dtype=np.int32), 10)
    with pytest.raises(codec.CodecError, match="n_classes"):
        codec.check_labels(np.asarray([1], dtype=np.int32), None)


def _example_groups(rng, with_labels):
    groups = []
    for n in (3, 3, 2):
        words = [rng.integers(0, 1 << 32, int(rng.integers(2, 40)), dtype=np.uint64).astype(np.uint32) for _ in range(n)]
        groups.append((rng.integers(0, 10, n).astype(np.int32) if with_labels else None, words))
    return groups


@pytest.mark.parametrize("with_labels", [False, True])
def test_container_round_trip(with_labels):
    from dynamicvectorquantization_amd import codec
    groups = _example_groups(np.random.default_rng(3), with_labels)
    fp = bytes(range(8))
    blob = codec.pack_container(groups, 3, fp, 1, 1, 4, 8, with_labels)
    assert blob == cm.pack(groups, 3, fp, 1, 1, 4, 8, with_labels)       # the package and the restatement write the same bytes
    for header, got in (codec.parse_container(blob), cm.parse(blob)):
        assert header["group_size"] == 3 and header["n_images"] == 8 and header["fingerprint"] == fp
        assert header["coarse_hw"] == 4 and header["fine_hw"] == 8 and header["with_labels"] == with_labels
        assert len(got) == len(groups)
        for (la, wa), (lb, wb) in zip(groups, got):
            assert (la is None and lb is None) or np.array_equal(la, lb)
            assert len(wa) == len(wb) and all(np.array_equal(a, b) for a, b in zip(wa, wb))
    header, _ = codec.parse_container(blob)
    assert header["dtype"] == "bf16" and header["step"] == 1
    assert codec.payload_bits(blob).tolist() == [32 * len(w) for _, ws in groups for w in ws]
    codec.check_header(header, fp, "bf16", 1, 4, 8, with_labels)
    empty = codec.pack_container([], 3, fp, 0, 0, 4, 8, with_labels)
    assert codec.parse_container(empty)[1] == [] and empty == cm.pack([], 3, fp, 0, 0, 4, 8, with_labels)


def test_container_rejections():
    """a truncated blob, a flipped payload byte, bad magic, a wrong fingerprint (and dtype): CodecError from the host-side checks --
    parse_container and check_header import no torch and touch no GPU"""
    from dynamicvectorquantization_amd import codec
    groups = _example_groups(np.random.default_rng(4), True)
    fp = b"\x01\x02\x03\x04\x05\x06\x07\x08"
    blob = codec.pack_container(groups, 3, fp, 1, 0, 4, 8, True)
    codec.parse_container(blob)
    for cut in (0, 10, codec.HEADER_BYTES - 1, codec.HEADER_BYTES + 2, len(blob) // 2, len(blob) - 4, len(blob) - 1):
        with pytest.raises(codec.CodecError):
            codec.parse_container(blob[:cut])
        with pytest.raises(cm.ContainerError):
            cm.parse(blob[:cut])
    for at in (codec.HEADER_BYTES + 4 + 2, len(blob) // 2, len(blob) - 9, 9, 25):   # labels, words, last word, group size, fingerprint
        bad = bytearray(blob)
        bad[at] ^= 0x10
        with pytest.raises(codec.CodecError):
            codec.parse_container(bytes(bad))
        with pytest.raises(cm.ContainerError):
            cm.parse(bytes(bad))
    with pytest.raises(codec.CodecError, match="magic"):
        codec.parse_container(b"DQTX" + blob[4:])
    with pytest.raises(codec.CodecError, match="version"):
        head = bytearray(blob[:36])
        head[4] = 2
        codec.parse_container(bytes(head) + struct.pack("<I", zlib.crc32(bytes(head))) + blob[40:])
    with pytest.raises(codec.CodecError):
        codec.parse_container(blob + b"\0\0\0\0")
    # a count the model's loop could never produce, with a valid CRC
    huge = [(np.zeros(1, dtype=np.int32), [np.zeros(4 * 4 * 2 + 8 * 8 + 9, dtype=np.uint32)])]
    with pytest.raises(codec.CodecError, match="word count"):
        codec.parse_container(codec.pack_container(huge, 1, fp, 1, 0, 4, 8, True))
    header, _ = codec.parse_container(blob)
    with pytest.raises(codec.CodecError, match="fingerprint"):
        codec.check_header(header, b"\x09" * 8, "bf16", 0, 4, 8, True)
    with pytest.raises(codec.CodecError, match="compute dtype"):
        codec.check_header(header, fp, "fp32", 0, 4, 8, True)
    with pytest.raises(codec.CodecError, match="geometry"):
        codec.check_header(header, fp, "bf16", 0, 16, 32, True, force=True)
    codec.check_header(header, b"\x09" * 8, "fp32", 0, 4, 8, True, force=True)     # force lets fingerprint and dtype pass
