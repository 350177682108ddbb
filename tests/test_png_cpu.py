"""CPU: the host side of the device PNG decode (docs/design/29-device-png.md) and of the FFHQ data path -- the test writer and the numpy
restatement of the un-filtering against PIL, data.decode_png_host (what it takes, what it refuses and why, that it never raises), the
FFHQ dataset class, the crop-a-box-then-resize plan against PIL, the box sampler.  Exact equality everywhere."""
import io
import struct
import zlib

import numpy as np
import pytest

import png_math as pm
from dynamicvectorquantization_amd import data as D
from oracle import data as odata

CASES = pm.cases()


def test_case_matrix_covers_the_edges():
    ws, hs = {c[1].shape[1] for c in CASES}, {c[1].shape[0] for c in CASES}
    assert {1, 2, 3, 5, 63, 64, 65, 257} <= ws and {1, 2, 63, 64, 65, 129} <= hs and {c[1].shape[2] for c in CASES} == {1, 2, 3, 4}
    assert all(c[1].shape[1] < 260 and c[1].shape[0] < 130 for c in CASES) and 35 <= len(CASES) <= 50
    assert {int(f) for c in CASES for f in c[2]} == {0, 1, 2, 3, 4}


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_writer_restatement_and_host_pass_equal_pil(case):
    name, pix, filters, nidat = case
    data = pm.write_png(pix, filters, nidat)
    ref = pm.pil_rgb(data)
    assert np.array_equal(ref, pm.to_rgb(pix)), "PIL does not decode the written file to the pixels it was written from"
    h, w, bpp = pix.shape
    assert D.png_info(data) == (True, "ok")
    rec = D.decode_png_host(data)
    assert (rec["w"], rec["h"], rec["bpp"]) == (w, h, bpp) and rec["scan"].dtype == np.uint8 and rec["scan"].size == h * (1 + w * bpp)
    assert np.array_equal(rec["scan"], pm.filter_rows(pix, filters))           # the scanlines stay FILTERED on the host
    assert np.array_equal(pm.to_rgb(pm.unfilter(rec["scan"], w, h, bpp)), ref)


def test_directed_cases_hit_what_they_are_for():
    by = {c[0]: c for c in CASES}
    t = by["paeth-ties"][1].astype(np.int64)
    a, b, c = t[1:, :-1], t[:-1, 1:], t[:-1, :-1]
    p = a + b - c
    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
    assert (pa == pb).any() and ((pa == pc) & (pa < pb) & (a != c)).any() and ((pb == pc) & (pb < pa) & (b != c)).any()
    t = by["average-carry"][1].astype(np.int64)
    assert (t[1:, :-1] + t[:-1, 1:] >= 256).all()
    assert set(np.unique(by["wrap-0-255"][1])) == {0, 255}


def _refusals():
    pix = pm.picture(9, 7, 3, 1)
    good = pm.write_png(pix, [0, 1, 2, 3, 4, 1, 2], 2)
    scan = pm.filter_rows(pix, [0, 1, 2, 3, 4, 1, 2])
    flipped = bytearray(good)
    flipped[-20] ^= 0x10                                            # inside the last IDAT: its CRC no longer matches
    bad5 = scan.copy()
    bad5[3 * (1 + 27)] = 5
    adler = bytearray(zlib.compress(scan.tobytes()))
    adler[-1] ^= 1
    from PIL import Image
    pal, jpg, bit1, d16 = io.BytesIO(), io.BytesIO(), io.BytesIO(), io.BytesIO()
    Image.fromarray(pix, "RGB").quantize(16).save(pal, "PNG")
    Image.fromarray(pix, "RGB").save(jpg, "JPEG")
    Image.fromarray(pix[..., 0] > 127).save(bit1, "PNG")
    Image.fromarray(pix[..., 0].astype(np.uint16) * 257).save(d16, "PNG")
    return good, [
        ("palette", pal.getvalue(), "palette"),
        ("16-bit", d16.getvalue(), "bit depth"),
        ("1-bit", bit1.getvalue(), "bit depth"),
        ("interlaced", pm.assemble(9, 7, 2, zlib.compress(scan.tobytes()), interlace=1), "interlaced"),
        ("apng", pm.write_png(pix, [0] * 7, extra=[pm.chunk(b"acTL", struct.pack(">II", 1, 0))]), "APNG"),
        ("crc", bytes(flipped), "bad CRC"),
        ("filter-5", pm.assemble(9, 7, 2, zlib.compress(bad5.tobytes())), "filter type"),
        ("one-row-short", pm.assemble(9, 7, 2, zlib.compress(scan[:-28].tobytes())), "stream length"),
        ("one-byte", pm.assemble(9, 7, 2, zlib.compress(b"\x00")), "stream length"),
        ("one-byte-over", pm.assemble(9, 7, 2, zlib.compress(scan.tobytes() + b"\x00")), "stream length"),
        ("adler", pm.assemble(9, 7, 2, bytes(adler)), "zlib error"),
        ("cut-stream", pm.assemble(9, 7, 2, zlib.compress(scan.tobytes())[:-2]), "stream not finished"),
        ("idat-apart", good[:33] + pm.chunk(b"IDAT", zlib.compress(scan.tobytes())[:10]) + pm.chunk(b"tEXt", b"k\x00v")
         + pm.chunk(b"IDAT", zlib.compress(scan.tobytes())[10:]) + pm.chunk(b"IEND"), "IDAT chunks not consecutive"),
        ("jpeg", jpg.getvalue(), "not a PNG"),
        ("empty", b"", "not a PNG"),
    ]


def test_refusals_and_their_reasons():
    good, bad = _refusals()
    assert D.png_info(good) == (True, "ok")
    for name, data, reason in bad:
        assert D.png_info(data) == (False, reason), name
        assert D.decode_png_host(data) is None, name
    # 16-bit and 1-bit files written by PIL really are what their names say
    assert bad[1][1][24] == 16 and bad[2][1][24] == 1 and bad[0][1][25] == 3


def test_ancillary_chunks_do_not_change_the_pixels():
    """tRNS on a grey and an RGB file, gAMA: PIL's RGB pixels are the file's samples, and the host pass takes the files"""
    for bpp, trns in ((1, struct.pack(">H", 7)), (3, struct.pack(">HHH", 1, 2, 3))):
        pix = pm.picture(11, 6, bpp, 5)
        data = pm.write_png(pix, [4, 3, 2, 1, 0, 4], extra=[pm.chunk(b"gAMA", struct.pack(">I", 45455)), pm.chunk(b"tRNS", trns)])
        rec = D.decode_png_host(data)
        assert rec is not None and np.array_equal(pm.to_rgb(pm.unfilter(rec["scan"], 11, 6, bpp)), pm.pil_rgb(data))


def test_truncation_never_raises_and_never_decodes():
    good, _ = _refusals()
    for n in range(len(good)):
        assert D.decode_png_host(good[:n]) is None, n
    assert D.decode_png_host(good) is not None
    assert D.decode_png_host(good + b"trailing bytes") is not None


def test_inflate_is_bounded(monkeypatch):
    """an IDAT stream that inflates to 100 x the declared size is refused after at most one byte more than the declared size"""
    w, h = 64, 64
    expected = h * (1 + 3 * w)
    bomb = pm.assemble(w, h, 2, zlib.compress(bytes(100 * expected), 9))
    seen = []
    real = zlib.decompressobj

    class Watched:
        def __init__(self):
            self.z = real()

        def decompress(self, data, max_length=0):
            out = self.z.decompress(data, max_length)
            seen.append((max_length, len(out)))
            return out

        @property
        def eof(self):
            return self.z.eof
    monkeypatch.setattr(D.zlib, "decompressobj", Watched)
    assert D.png_info(bomb) == (False, "stream length")
    assert seen == [(expected + 1, expected + 1)]


def test_example_kinds_and_loader_argument(tmp_path):
    from PIL import Image
    pix = pm.picture(20, 10, 3, 9)
    (tmp_path / "a.png").write_bytes(pm.write_png(pix, [4] * 10))
    Image.fromarray(pix, "RGB").quantize(8).save(tmp_path / "b.png")
    Image.fromarray(pix, "RGB").save(tmp_path / "c.jpg", quality=90)
    paths = [str(tmp_path / n) for n in ("a.png", "b.png", "c.jpg")]
    kinds = lambda ds: [sorted(set(ds[i]) & {"jpeg", "png", "image_u8"}) for i in range(3)]        # noqa: E731
    assert kinds(D.ImagePaths(paths)) == [["image_u8"]] * 3
    assert kinds(D.ImagePaths(paths, device_decode=True)) == [["image_u8"], ["image_u8"], ["jpeg"]]
    assert kinds(D.ImagePaths(paths, device_png=True)) == [["png"], ["image_u8"], ["image_u8"]]
    assert kinds(D.ImagePaths(paths, device_decode=True, device_png=True)) == [["png"], ["image_u8"], ["jpeg"]]
    ds = D.ImagePaths(paths)
    assert set(ds.example(0, False, True)) >= {"png", "file_path_"} and "image_u8" in ds.example(0, True)
    assert np.array_equal(ds[0]["image_u8"], pix)
    with pytest.raises(TypeError):
        D.GpuBatchLoader([1, 2], 1, "cpu", device_png=True)
    # layout: PNG records get slots like everything else, and descriptors of their own
    recs = [D.decode_png_host(paths[0]), ds[1]["image_u8"], D.decode_png_host(paths[0])]
    descs, coef_len, plane_len, rgb_len, offs, sizes = D.jpeg_batch_layout(recs)
    assert coef_len == 0 and offs == [0, 608, 1216] and rgb_len == 1824 and sizes == [(20, 10)] * 3
    pd, n, scan_len = D.png_batch_layout(recs, offs)
    assert n == 2 and scan_len == 2 * 10 * 61 and (pd[1].scan_off, pd[1].rgb_off, pd[1].w, pd[1].h, pd[1].bpp) == (610, 1216, 20, 10, 3)


def test_device_png_flags_parse():
    import importlib.util
    import os

    from conftest import REPO
    import train
    opt, _ = train.get_parser().parse_known_args(["-b", "x.yml", "--real_data", "--device_png"])
    assert opt.device_png and not opt.device_jpeg
    assert not train.get_parser().parse_known_args(["-b", "x.yml"])[0].device_png
    for name in ("tokenize_dataset", "eval_reconstruction", "calculate_entropy_thresholds", "codebook_usage_dqvae", "eval_likelihood"):
        src = open(os.path.join(REPO, "scripts", "tools", name + ".py")).read()
        assert "device_png=opt.device_png" in src or "opt.device_png)" in src, name
        spec = importlib.util.spec_from_file_location("dvq_png_flag_" + name, os.path.join(REPO, "scripts", "tools", name + ".py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        if hasattr(mod, "get_parser"):
            args = {"tokenize_dataset": ["--yaml_path", "x.yml", "--out", "o"], "calculate_entropy_thresholds": ["--images", "d"]}.get(
                name, ["--yaml_path", "x.yml"])
            assert mod.get_parser().parse_known_args(args + ["--device_png"])[0].device_png
            assert not mod.get_parser().parse_known_args(args)[0].device_png


# ---- FFHQ ------------------------------------------------------------------------------------------------------------------------
def _ffhq_tree(root, n=7, size=40):
    (root / "FFHQ").mkdir(parents=True)
    (root / "assets").mkdir()
    names = [f"{i:05d}.png" for i in range(n)]
    for i, name in enumerate(names):
        pix = pm.picture(size, size, 3, 70 + i)
        (root / "FFHQ" / name).write_bytes(pm.write_png(pix, np.random.default_rng(i).integers(0, 5, size=size)))
    (root / "FFHQ" / "notes.txt").write_text("not an image")
    (root / "assets" / "ffhqtrain.txt").write_text("".join(f"{n}\n" for n in names[:5]))
    (root / "assets" / "ffhqvalidation.txt").write_text("".join(f"{n}\n" for n in names[5:]))
    return names


def test_ffhq_splits_and_alias(tmp_path):
    from dynamicvectorquantization_amd import config as cfg
    names = _ffhq_tree(tmp_path)
    tr, va, tv = (D.FFHQ(split=s, root=str(tmp_path)) for s in ("train", "val", "trainval"))
    assert (len(tr), len(va), len(tv)) == (5, 2, 7)
    assert [p.split("/")[-1] for p in tr.paths] == names[:5] and sorted(p.split("/")[-1] for p in tv.paths) == names
    assert tr.is_train and tr.transform_kind == "random_resized_crop"
    assert not va.is_train and va.transform_kind is None
    ev = D.FFHQ(split="train", is_eval=True, root=str(tmp_path))
    assert not ev.is_train and ev.transform_kind is None and len(ev) == 5
    ex = tr[1]
    assert set(ex) == {"image_u8", "file_path_"} and ex["image_u8"].shape == (40, 40, 3)       # no class keys
    assert set(D.FFHQ(root=str(tmp_path), device_png=True)[1]) == {"png", "file_path_"}
    assert cfg.get_obj_from_str("data.faceshq.FFHQ") is D.FFHQ
    ds = cfg.instantiate_from_config({"target": "data.faceshq.FFHQ", "params": {"split": "val", "root": str(tmp_path)}})
    assert len(ds) == 2
    other = tmp_path / "mylist.txt"
    other.write_text(names[6] + "\n")
    assert len(D.FFHQ(split="train", root=str(tmp_path), train_list_file=str(other))) == 1
    with pytest.raises(ValueError):
        D.FFHQ(split="test", root=str(tmp_path))


def test_ffhq_missing_root_says_which_key(tmp_path):
    for root in (None, str(tmp_path / "nowhere")):
        with pytest.raises(FileNotFoundError, match="root"):
            D.FFHQ(root=root)


def test_ffhq_config_is_the_entropy_dual_config_on_ffhq():
    import os

    from conftest import REPO
    from dynamicvectorquantization_amd import config as cfg
    ours = cfg.load_yaml(os.path.join(REPO, "configs", "stage1", "dqvae-entropy-dual-r05_ffhq.yml"))
    base = cfg.load_yaml(os.path.join(REPO, "configs", "stage1", "dqvae-entropy-dual-r05_imagenet.yml"))
    p = ours.data.params
    assert p.train.target == p.validation.target == "data.faceshq.FFHQ"
    assert (p.train.params.split, p.validation.params.split) == ("train", "val") and p.train.params.root is None
    router = ours.model.params.encoderconfig.params.router_config.params
    assert router.json_path.endswith("entropy_thresholds_ffhq_train_patch-16.json") and os.path.exists(os.path.join(REPO, router.json_path))
    # everything but the data section and the thresholds file is the shipped entropy-dual config
    a, b = cfg.to_plain(ours), cfg.to_plain(base)
    a["model"]["params"]["encoderconfig"]["params"]["router_config"]["params"].pop("json_path")
    b["model"]["params"]["encoderconfig"]["params"]["router_config"]["params"].pop("json_path")
    assert a["model"] == b["model"] and a["data"]["params"]["batch_size"] == b["data"]["params"]["batch_size"]


# ---- the crop-a-box-then-resize plan ---------------------------------------------------------------------------------------------
def _apply_plan(plan, i, img):
    """image i of a plan through the numpy arithmetic of the resize (oracle.data._pass), reading the plan's OWN tables as the kernels
    do: absolute source indices, the horizontal pass on source rows [row0, row0 + rows), the vertical pass on that intermediate"""
    S = plan["size"]
    d = (D._Desc * plan["batch"]).from_buffer_copy(plan["desc"].tobytes())[i]
    tab = plan["tab"]
    hb = tab[d.hb_off:d.hb_off + 2 * S].reshape(S, 2)
    hk = tab[d.hk_off:d.hk_off + S * d.hks].reshape(S, d.hks)
    vb = tab[d.vb_off:d.vb_off + 2 * S].reshape(S, 2)
    vk = tab[d.vk_off:d.vk_off + S * d.vks].reshape(S, d.vks)
    assert hb[:, 0].min() >= 0 and (hb[:, 0] + hb[:, 1]).max() <= d.w and d.row0 >= 0 and d.row0 + d.rows <= d.h
    assert vb[:, 0].min() >= d.row0 and (vb[:, 0] + vb[:, 1]).max() <= d.row0 + d.rows
    t = odata._pass(img[d.row0:d.row0 + d.rows], [(int(x0), [int(v) for v in hk[x, :n]]) for x, (x0, n) in enumerate(hb)])
    out = odata._pass(t.transpose(1, 0, 2), [(int(y0) - d.row0, [int(v) for v in vk[y, :n]]) for y, (y0, n) in enumerate(vb)])
    out = out.transpose(1, 0, 2)
    return out[:, ::-1] if d.flip else out


BOXES = [((90, 70), (0, 0, 90, 70), 32), ((90, 70), (13, 5, 60, 60), 32), ((90, 70), (29, 9, 61, 61), 64), ((64, 64), (7, 11, 57, 53), 64),
         ((130, 131), (1, 2, 128, 129), 32), ((50, 50), (49, 0, 1, 50), 16), ((40, 40), (3, 3, 16, 16), 16)]


def test_box_plan_equals_pil_crop_then_resize():
    from PIL import Image
    imgs = [pm.picture(w, h, 3, 600 + i) for i, ((w, h), _, _) in enumerate(BOXES)]
    for size in sorted({s for _, _, s in BOXES}):
        sel = [i for i, b in enumerate(BOXES) if b[2] == size]
        flips = [bool(k % 2) for k in range(len(sel))]
        plan = D.plan_batch([imgs[i] for i in sel], size, boxes=[BOXES[i][1] for i in sel], flips=flips)
        for k, i in enumerate(sel):
            left, top, bw, bh = BOXES[i][1]
            ref = np.asarray(Image.fromarray(imgs[i], "RGB").crop((left, top, left + bw, top + bh)).resize((size, size), Image.BILINEAR))
            ref = ref[:, ::-1] if flips[k] else ref
            assert np.array_equal(_apply_plan(plan, k, imgs[i]), ref), BOXES[i]
    # without a box the plan is what it was: the same tables as a whole-image box gives after Resize's own geometry
    a, b = D.plan_batch_sizes([(64, 64)], 32), D.plan_batch_sizes([(64, 64)], 32, boxes=[(0, 0, 64, 64)])
    assert np.array_equal(a["tab"], b["tab"]) and np.array_equal(a["desc"], b["desc"])
    with pytest.raises(AssertionError):
        D.plan_batch_sizes([(64, 64)], 32, boxes=[(10, 0, 60, 60)])


def test_box_sampler_bounds_and_fallback():
    rng = np.random.default_rng(5)
    sides = set()
    for w in (256, 1024, 40, 7, 1):
        area = w * w
        for _ in range(200):
            left, top, bw, bh = D.sample_square_box(w, w, rng)
            assert bw == bh and 0 <= left and 0 <= top and left + bw <= w and top + bh <= w
            # side = round(sqrt(t)) with 0.75 area <= t <= area: the square of a rounded root is within side + 1/4 of t
            assert 0.75 * area - bw - 0.25 <= bw * bh <= area
            sides.add((w, bw))
    assert len({s for w, s in sides if w == 1024}) > 50          # the scale is drawn, not fixed
    # a target square never fits a 2:1 image (sqrt(0.75 * 2) > 1): the centred square of the short side, after 10 draws
    rng = np.random.default_rng(6)
    state = rng.bit_generator.state
    assert D.sample_square_box(100, 50, rng) == (25, 0, 50, 50) and D.sample_square_box(50, 101, rng) == (0, 25, 50, 50)
    rng2 = np.random.default_rng(6)
    rng2.bit_generator.state = state
    for _ in range(10):
        rng2.uniform(0.75, 1.0)
    rng3 = np.random.default_rng(6)
    rng3.bit_generator.state = state
    D.sample_square_box(100, 50, rng3)
    assert rng2.random() == rng3.random()                      # exactly 10 tries were drawn
    # the plan draws the box, then the flip, from the loader's generator
    plan = D.plan_batch_sizes([(80, 80)] * 6, 16, train=True, rng=np.random.default_rng(1), rrc=D.RRC_SCALE)
    r = np.random.default_rng(1)
    for d in (D._Desc * 6).from_buffer_copy(plan["desc"].tobytes()):
        left, top, side, _ = D.sample_square_box(80, 80, r)
        assert d.flip == int(r.random() < 0.5) and d.row0 == top and d.rows == side
