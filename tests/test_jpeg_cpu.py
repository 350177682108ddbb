"""CPU tests of the device JPEG decode (docs/design/23-device-jpeg.md): the numpy restatement of its arithmetic (tests/jpeg_math.py) equals
PIL pixel for pixel, the library's host pass (dvq_jpeg_info, dvq_jpeg_entropy_decode) equals the restatement's slow Huffman decoder
coefficient for coefficient, refuses what it does not take with the reason, and survives damaged input; the flags parse.  Every
comparison is exact: the arithmetic is integer."""
import ctypes as C
import importlib.util
import io
import os
import sys

import numpy as np
import pytest

import jpeg_math as jm
from conftest import REPO

NAMES = [c[0] for c in jm.CASES]


@pytest.fixture(scope="module")
def lib():
    from dynamicvectorquantization_amd import _lib, build
    build.build(verbose=False)
    return _lib.load()


def _info(lib, data):
    from dynamicvectorquantization_amd import _lib
    info = _lib.JpegInfo()
    assert lib.dvq_jpeg_info(data, len(data), C.byref(info)) == 0
    return info


def _host_decode(lib, data, capacity=None, guard=64):
    """-> (return code, coef int16 [count], qtab uint16 [ncomp, 64]); the words behind `capacity` must come back untouched"""
    info = _info(lib, data)
    count = info.coef_count if capacity is None else capacity
    coef = np.full(count + guard, 0x5A5A, dtype=np.int16)
    qtab = np.zeros((max(1, info.components), 64), dtype=np.uint16)
    rc = lib.dvq_jpeg_entropy_decode(data, len(data), coef.ctypes.data, count, qtab.ctypes.data)
    assert (coef[count:] == 0x5A5A).all(), "dvq_jpeg_entropy_decode wrote past coef_capacity"
    return rc, coef[:count], qtab


@pytest.mark.parametrize("name", NAMES)
def test_restatement_equals_pil(name):
    from PIL import features
    assert features.check_feature("libjpeg_turbo"), "the acceptance bar is libjpeg-turbo's default decode path"
    data = jm.case_bytes(name)
    assert np.array_equal(jm.decode(data), jm.pil_rgb(data))


@pytest.mark.parametrize("name", NAMES)
def test_info_and_coefficients(lib, name):
    from PIL import Image

    from dynamicvectorquantization_amd import _lib
    data = jm.case_bytes(name)
    _, w, h, mode, opts = jm.CASES[NAMES.index(name)]
    info = _info(lib, data)
    with Image.open(io.BytesIO(data)) as im:
        assert (info.width, info.height) == im.size == (w, h)
        assert info.components == {"L": 1, "RGB": 3}[im.mode] and im.mode == mode
    assert info.supported == _lib.JPEG_SUPPORTED
    assert info.coef_count == jm.coef_count(data)
    hdr = jm.parse(data)
    nc, hs, vs = jm.geometry(hdr)[:3]
    assert (info.h_samp[0], info.v_samp[0]) == (hs, vs) and all((info.h_samp[c], info.v_samp[c]) == (1, 1) for c in range(1, nc))
    assert [info.qtab_index[c] for c in range(nc)] == [comp[3] for comp in hdr["comps"]]
    assert info.restart_interval == hdr["ri"]
    if "restart_marker_blocks" in opts:
        assert info.restart_interval == opts["restart_marker_blocks"]
    rc, coef, qtab = _host_decode(lib, data)
    assert rc == 0, lib.dvq_last_error()
    ref_coef, ref_q = jm.entropy_decode(data)
    assert np.array_equal(coef, np.concatenate([c.reshape(-1) for c in ref_coef]))
    assert np.array_equal(qtab, ref_q)


def _patched_sampling(data, hv):
    i = data.index(b"\xff\xc0")
    out = bytearray(data)
    out[i + 11] = hv          # marker 2, length 2, precision 1, height 2, width 2, components 1, id 1 -> the luma sampling byte
    return bytes(out)


def test_refusals_carry_their_reason(lib):
    from PIL import Image

    from dynamicvectorquantization_amd import _lib
    from dynamicvectorquantization_amd import data as D
    rgb = jm.test_image(40, 30, "RGB", 3)

    def saved(im, fmt, **opts):
        buf = io.BytesIO()
        im.save(buf, fmt, **opts)
        return buf.getvalue()
    cases = [
        (saved(Image.fromarray(rgb, "RGB"), "JPEG", progressive=True), _lib.JPEG_PROGRESSIVE),
        (saved(Image.fromarray(rgb, "RGB").convert("CMYK"), "JPEG"), _lib.JPEG_COMPONENTS),
        (saved(Image.fromarray(rgb, "RGB"), "PNG"), _lib.JPEG_NOT_JPEG),
        (_patched_sampling(jm.case_bytes("45x37_420"), 0x41), _lib.JPEG_SAMPLING),
        (b"", _lib.JPEG_NOT_JPEG),
        (jm.case_bytes("45x37_420")[:100], _lib.JPEG_MALFORMED),
    ]
    for data, reason in cases:
        info = _info(lib, data)
        assert info.supported == reason and info.coef_count == 0
        coef, q = np.zeros(64, dtype=np.int16), np.zeros((4, 64), dtype=np.uint16)
        assert lib.dvq_jpeg_entropy_decode(data, len(data), coef.ctypes.data, 64, q.ctypes.data) == -1
        assert b"not a supported JPEG" in lib.dvq_last_error()
        assert D.decode_jpeg_host(data) is None
    assert lib.dvq_jpeg_info(None, 0, None) == -1 and b"null" in lib.dvq_last_error()
    # the progressive and the CMYK file still report their frame
    assert (_info(lib, cases[0][0]).width, _info(lib, cases[0][0]).height) == (40, 30) and _info(lib, cases[1][0]).components == 4


def test_truncation_at_every_offset_and_small_capacity(lib):
    data = jm.case_bytes("45x37_420")
    full = _host_decode(lib, data)
    assert full[0] == 0
    scan_off = jm.parse(data)["scan_off"]
    outcomes = set()
    for n in range(len(data)):
        cut = data[:n]
        info = _info(lib, cut)
        if n < scan_off:
            assert info.supported != 0
        rc, coef, _ = _host_decode(lib, cut, capacity=int(full[1].size))
        assert rc in (0, -1), (n, rc)
        outcomes.add(rc)
        if rc == 0:               # only the end-of-image marker (and padding bits) may be missing
            assert n >= len(data) - 3 and np.array_equal(coef, full[1])
        else:
            assert lib.dvq_last_error()
    assert outcomes == {0, -1}
    # the restart file: cut inside intervals and inside the markers between them
    rst = jm.case_bytes("64x48_rst3")
    for n in range(jm.parse(rst)["scan_off"], len(rst) - 2):
        assert _host_decode(lib, rst[:n], capacity=jm.coef_count(rst))[0] == -1
    # a buffer that is too small: refused before anything is written
    rc, coef, _ = _host_decode(lib, data, capacity=int(full[1].size) - 1)
    assert rc == -5 and b"coef_capacity" in lib.dvq_last_error() and (coef == 0x5A5A).all()
    # a corrupted entropy segment: never a crash, never a write outside
    rng = np.random.default_rng(0)
    for _ in range(200):
        bad = bytearray(data)
        for k in rng.integers(scan_off, len(data), size=3):
            bad[k] = int(rng.integers(0, 256))
        assert _host_decode(lib, bytes(bad))[0] in (0, -1)


def _sos_offset(data):
    pos = 2
    while True:
        while data[pos] == 0xFF:
            pos += 1
        m = data[pos]
        pos += 1
        if m == 0xDA:
            return pos - 2
        if m == 0x01 or 0xD0 <= m <= 0xD8:
            continue
        pos += (data[pos] << 8) | data[pos + 1]


def _with_segment(data, marker, payload):
    """one more segment in front of the SOS: a later table definition replaces an earlier one"""
    sos = _sos_offset(data)
    n = len(payload) + 2
    return data[:sos] + bytes([0xFF, marker, n >> 8, n & 255]) + bytes(payload) + data[sos:]


def _dht(tc_th, counts):
    """a DHT payload: counts {length: codes}, values 0, 1, 2, ..."""
    bits = [counts.get(length, 0) for length in range(1, 17)]
    return [tc_th] + bits + [i & 255 for i in range(sum(bits))]


# more codes of a length than the length holds: at 1 bit, at the 9-bit lookahead's edge, beyond it
OVERSUBSCRIBED = [{1: 3}, {1: 6}, {1: 200}, {1: 2, 9: 5}, {1: 2, 10: 1}, {1: 2, 16: 1}, {1: 1, 8: 255}, {2: 4, 3: 1}]


@pytest.mark.parametrize("name", ["45x37_420", "31x29_grey"])
def test_wrong_but_well_formed_headers(lib, name):
    """segments whose own lengths are right and whose content is not: the table builder must refuse an over-subscribed Huffman table
    BEFORE a code indexes its lookahead table (6 codes of 1 bit once wrote past it), and nothing may be written outside the buffers"""
    from dynamicvectorquantization_amd import _lib
    from dynamicvectorquantization_amd import data as D
    data = jm.case_bytes(name)
    good = _host_decode(lib, data)
    assert good[0] == 0
    for tc_th in (0x00, 0x10):
        for counts in OVERSUBSCRIBED + [{}]:                     # {}: a table without codes
            bad = _with_segment(data, 0xC4, _dht(tc_th, counts))
            assert _info(lib, bad).supported == _lib.JPEG_SUPPORTED          # the markers are fine: the tables are built by the decode
            rc, coef, _ = _host_decode(lib, bad)
            assert rc == -1, (tc_th, counts)
            if counts:
                assert b"invalid" in lib.dvq_last_error() and b"Huffman table" in lib.dvq_last_error()
                assert (coef == 0x5A5A).all()                    # refused before the first coefficient
            assert D.decode_jpeg_host(bad) is None
    # exactly 256 codes (a complete code): symbols above 15 are no DC categories; as an AC table it builds, whatever the data then means
    full = {8: 255, 9: 1}
    assert _host_decode(lib, _with_segment(data, 0xC4, _dht(0x00, full)))[0] == -1
    assert _host_decode(lib, _with_segment(data, 0xC4, _dht(0x10, full)))[0] in (0, -1)
    # the luma quantisation table again with 16-bit entries: the same output; with a value above 255: reported as it is
    hdr = jm.parse(data)
    tq = hdr["comps"][0][3]
    zz = [int(hdr["q"][tq][jm.NATURAL[k]]) for k in range(64)]
    for vals in (zz, [1000] + zz[1:]):
        rc, coef, qtab = _host_decode(lib, _with_segment(data, 0xDB, [0x10 | tq] + [b for v in vals for b in (v >> 8, v & 255)]))
        assert rc == 0 and np.array_equal(coef, good[1]) and qtab[0, 0] == vals[0] and np.array_equal(qtab[0, 1:], good[2][0, 1:])
    # a scan that names Huffman tables nobody defined
    sos = _sos_offset(data)
    bad = bytearray(data)
    bad[sos + 6] = 0x33
    assert _info(lib, bytes(bad)).supported == _lib.JPEG_MALFORMED


def test_host_record_and_planning_from_sizes(lib):
    """decode_jpeg_host's record, and plan_batch_sizes == plan_batch on the same sizes, crops and flips (and the same draws in training)"""
    from dynamicvectorquantization_amd import data as D
    rec = D.decode_jpeg_host(jm.case_bytes("33x50_422"))
    assert (rec["w"], rec["h"], rec["ncomp"], rec["hs"], rec["vs"]) == (33, 50, 3, 2, 1)
    assert rec["coef"].dtype == np.int16 and rec["coef"].size == jm.coef_count(jm.case_bytes("33x50_422")) and rec["qtab"].shape == (3, 64)
    assert C.sizeof(D._JpegDesc) == lib.dvq_jpeg_desc_bytes() == 464
    imgs = [jm.test_image(300, 400, "RGB", 1), jm.test_image(333, 517, "RGB", 2), jm.test_image(256, 256, "RGB", 3)]
    sizes = [(im.shape[1], im.shape[0]) for im in imgs]
    for kw in (dict(crops=[(10, 0), (0, 31), (0, 0)], flips=[False, True, False]), dict(), dict(train=True)):
        a = D.plan_batch(imgs, 256, rng=np.random.default_rng(5), **kw)
        b = D.plan_batch_sizes(sizes, 256, rng=np.random.default_rng(5), **kw)
        assert "src" not in b and all(np.array_equal(a[k], b[k]) for k in b)
    offs = [0, 1 << 20, 1 << 21]
    descs = (D._Desc * 3).from_buffer_copy(D.plan_batch_sizes(sizes, 256, src_offs=offs)["desc"].tobytes())
    assert [d.src_off for d in descs] == offs


def test_dataset_hands_over_records_only_when_asked(tmp_path):
    from PIL import Image

    from dynamicvectorquantization_amd import data as D
    (tmp_path / "a.jpg").write_bytes(jm.case_bytes("45x37_420"))
    Image.fromarray(jm.test_image(20, 12, "RGB", 1), "RGB").save(tmp_path / "b.png")
    paths = [str(tmp_path / "a.jpg"), str(tmp_path / "b.png")]
    off, on = D.ImagePaths(paths), D.ImagePaths(paths, device_decode=True)
    assert set(off[0]) == {"image_u8", "file_path_"} and "jpeg" in on[0] and "image_u8" not in on[0]
    assert "image_u8" in on[1] and np.array_equal(on[1]["image_u8"], off[1]["image_u8"])        # the PNG: PIL, as before
    assert "jpeg" in off.example(0, True)
    with pytest.raises(TypeError):
        D.GpuBatchLoader([1, 2], 1, "cpu", device_decode=True)


def _script(name):
    spec = importlib.util.spec_from_file_location("dvq_script_" + name, os.path.join(REPO, "scripts", "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_device_jpeg_flags_parse(monkeypatch, capsys):
    sys.path.insert(0, REPO)
    import train
    opt, _ = train.get_parser().parse_known_args(["-b", "x.yml", "--real_data", "--device_jpeg"])
    assert opt.device_jpeg and opt.real_data
    assert not train.get_parser().parse_known_args(["-b", "x.yml"])[0].device_jpeg
    tok = _script("tokenize_dataset").get_parser()
    assert tok.parse_known_args(["--yaml_path", "x.yml", "--out", "o", "--device_jpeg"])[0].device_jpeg
    assert not tok.parse_known_args(["--yaml_path", "x.yml", "--out", "o"])[0].device_jpeg
    cal = _script("calculate_entropy_thresholds").get_parser()
    assert cal.parse_known_args(["--images", "d", "--device_jpeg"])[0].device_jpeg and not cal.parse_known_args([])[0].device_jpeg
    # the two evaluation scripts build their parser inside main(): their help names the flag, and they hand it to the loader
    for name in ("eval_reconstruction", "codebook_usage_dqvae"):
        mod = _script(name)
        monkeypatch.setattr(sys, "argv", [name + ".py", "--help"])
        with pytest.raises(SystemExit) as e:
            mod.main()
        assert e.value.code == 0 and "--device_jpeg" in capsys.readouterr().out
        assert "device_decode=opt.device_jpeg" in open(os.path.join(REPO, "scripts", "tools", name + ".py")).read()
