"""GPU tests of the device PNG decode and the FFHQ data path (docs/design/29-device-png.md): dvq_png_batch_unfilter against PIL on files
written with a chosen filter per row (tests/png_math.py); batches that mix JPEG records, PNG records and decoded arrays; the loader with
device_png against the loader without; evaluate.image_batches; FFHQ's crop-a-box-then-resize transform against PIL; train.py on the FFHQ
config.  Exact equality everywhere: the arithmetic is integer."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import jpeg_math as jm
import png_math as pm
from dynamicvectorquantization_amd import data as D
from dynamicvectorquantization_amd.kernels import _p, _s, check, lib
from oracle import data as odata

pytestmark = pytest.mark.gpu


def _images(out):
    rgb = out["rgb"].cpu().numpy()
    return [rgb[o:o + h * w * 3].reshape(h, w, 3) for o, (w, h) in zip(out["offs"], out["sizes"])]


def test_batch_unfilter_equals_pil(dev):
    """the whole case matrix in ONE launch: every width, height, bpp and filter of png_math.cases(), the three-band images first so that
    everything after them sits at large offsets, a host-decoded image between them.  The library is called on a buffer filled with a
    pattern: every image equals PIL's, and no byte outside the PNG slots (slot padding, the array's slot, the tail) is written"""
    cases = sorted(pm.cases(), key=lambda c: -c[1].size)
    datas = [pm.write_png(pix, filters, nidat) for _, pix, filters, nidat in cases]
    records = [D.decode_png_host(d) for d in datas]
    assert all(r is not None for r in records)
    extra = jm.test_image(21, 13, "RGB", 99)
    records.insert(3, extra)
    refs = [pm.pil_rgb(d) for d in datas]
    refs.insert(3, extra)
    assert C.sizeof(D._PngDesc) == lib().dvq_png_desc_bytes() == 32
    _, _, _, rgb_len, offs, sizes = D.jpeg_batch_layout(records)
    descs, n, scan_len = D.png_batch_layout(records, offs)
    assert n == len(cases) and all(o % 16 == 0 for o in offs)
    scan = torch.from_numpy(np.concatenate([r["scan"] for r in records if isinstance(r, dict)])).to(dev)
    assert scan.numel() == scan_len
    desc = torch.from_numpy(np.frombuffer(bytes(descs), dtype=np.uint8).copy()).to(dev)
    rgb = torch.full((rgb_len + 64,), 0xA5, dtype=torch.uint8, device=dev)
    check(lib().dvq_png_batch_unfilter(_p(scan), _p(desc), n, _p(rgb), _s()), "dvq_png_batch_unfilter")
    torch.cuda.synchronize()
    got = rgb.cpu().numpy()
    written = np.zeros(got.size, dtype=bool)
    for i, (o, (w, h), ref) in enumerate(zip(offs, sizes, refs)):
        if i == 3:
            continue
        g = got[o:o + h * w * 3].reshape(h, w, 3)
        written[o:o + h * w * 3] = True
        name = cases[i - (i > 3)][0]
        assert g.shape == ref.shape and np.array_equal(g, ref), f"{name}: {(g != ref).sum()} bytes differ from PIL"
    assert (got[~written] == 0xA5).all(), "bytes outside the PNG slots were written"
    # the public path: the same batch through decode_batch_gpu, which also copies the host-decoded image into its slot
    out = D.decode_batch_gpu(records, dev)
    torch.cuda.synchronize()
    assert out["offs"] == offs and out["sizes"] == sizes
    for g, ref in zip(_images(out), refs):
        assert np.array_equal(g, ref)


def _palette_png(w, h, seed):
    import io

    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(pm.picture(w, h, 3, seed), "RGB").quantize(32).save(buf, "PNG")
    return buf.getvalue()


def test_mixed_batch_of_jpeg_png_and_decoded_arrays(dev):
    from PIL import features
    if not features.check_feature("libjpeg_turbo"):
        pytest.fail("PIL without libjpeg-turbo: the JPEG slots have no oracle here")
    jpegs = [jm.case_bytes(n) for n in ("45x37_420", "31x29_grey", "40x24_444")]
    rng = np.random.default_rng(8)
    pngs = [pm.write_png(pm.picture(w, h, bpp, 20 + bpp), rng.integers(0, 5, size=h), 1 + bpp % 2)
            for w, h, bpp in ((70, 66, 1), (33, 129, 2), (129, 65, 3), (64, 64, 4))]
    pal = _palette_png(50, 41, 3)
    assert D.decode_png_host(pal) is None and D.png_info(pal) == (False, "palette")
    refs = [jm.pil_rgb(jpegs[0]), pm.pil_rgb(pngs[0]), pm.pil_rgb(pngs[1]), jm.pil_rgb(jpegs[1]), pm.pil_rgb(pal), pm.pil_rgb(pngs[2]),
            jm.pil_rgb(jpegs[2]), pm.pil_rgb(pngs[3])]
    records = [D.decode_jpeg_host(jpegs[0]), D.decode_png_host(pngs[0]), D.decode_png_host(pngs[1]), D.decode_jpeg_host(jpegs[1]),
               pm.pil_rgb(pal), D.decode_png_host(pngs[2]), D.decode_jpeg_host(jpegs[2]), D.decode_png_host(pngs[3])]
    assert all(r is not None for r in records)
    out = D.decode_batch_gpu(records, dev)
    torch.cuda.synchronize()
    for i, (g, ref) in enumerate(zip(_images(out), refs)):
        assert g.shape == ref.shape and np.array_equal(g, ref), f"slot {i}: {(g != ref).sum()} bytes differ from PIL"


def _folder(tmp_path, split="val"):
    """<tmp>/<split>/<class>/...: RGB, RGBA, grey, grey + alpha and palette PNGs (PIL's encoder chooses the filters here), one written
    with a chosen filter mix, one JPEG"""
    from PIL import Image
    specs = [("n01", "a.png", 90, 70, "RGB"), ("n01", "b.png", 64, 100, "RGBA"), ("n01", "c.png", 81, 67, "L"), ("n01", "d.png", 70, 70, "P"),
             ("n02", "e.jpg", 75, 66, "RGB"), ("n02", "f.png", 77, 93, "LA"), ("n02", "g.png", 66, 65, "own"), ("n02", "h.png", 120, 71, "RGB")]
    for i, (c, f, w, h, mode) in enumerate(specs):
        d = tmp_path / split / c
        d.mkdir(parents=True, exist_ok=True)
        bpp = {"RGB": 3, "RGBA": 4, "L": 1, "LA": 2, "P": 3, "own": 3}[mode]
        pix = pm.picture(w, h, bpp, 40 + i)
        if mode == "own":
            (d / f).write_bytes(pm.write_png(pix, np.random.default_rng(i).integers(0, 5, size=h), 2))
        elif mode == "P":
            Image.fromarray(pix, "RGB").quantize(64).save(d / f)
        elif f.endswith(".jpg"):
            Image.fromarray(pix, "RGB").save(d / f, quality=90)
        else:
            Image.fromarray(pix[..., 0] if bpp == 1 else pix, mode).save(d / f)
    return str(tmp_path / split)


KINDS_PNG = [{"png"}] * 3 + [{"image_u8"}] * 2 + [{"png"}] * 3                # the palette file and the JPEG stay with PIL


def test_loader_parity_eval_and_train(dev, tmp_path):
    root = _folder(tmp_path)
    kinds = lambda **kw: [set(D.ImageFolder(root, **kw)[i]) & {"jpeg", "png", "image_u8"} for i in range(8)]      # noqa: E731
    assert kinds(device_png=True) == KINDS_PNG
    assert kinds(device_decode=True) == [{"image_u8"}] * 4 + [{"jpeg"}] + [{"image_u8"}] * 3       # what they are today: JPEG only
    assert kinds(device_decode=True, device_png=True) == [{"png"}] * 3 + [{"image_u8"}, {"jpeg"}] + [{"png"}] * 3

    def batches(train, seed=3, **kw):
        ds = D.ImageFolder(root, is_train=train)
        loader = D.GpuBatchLoader(ds, 4, dev, size=64, shuffle=train, num_workers=2, seed=seed, **kw)
        return [{k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in b.items()} for b in loader]
    for train in (False, True):
        a = batches(train)
        for kw in (dict(device_png=True), dict(device_png=True, device_decode=True)):
            b = batches(train, **kw)
            assert len(a) == len(b) == 2
            for x, y in zip(a, b):
                assert set(x) == set(y) and x["image"].shape == (4, 3, 64, 64)
                assert np.array_equal(x["image"], y["image"]), f"train={train} {kw}: {(x['image'] != y['image']).sum()} elements differ"
                assert np.array_equal(x["class_label"], y["class_label"]) and list(x["relpath"]) == list(y["relpath"])
    # the eval batches are what PIL and the host oracle give for the files
    ds = D.ImageFolder(root)
    for bi, b in enumerate(batches(False, device_png=True)):
        for k in range(4):
            assert np.array_equal(b["image"][k], odata.reference_transform(ds[4 * bi + k]["image_u8"], 64))


def test_image_batches_see_the_same_pixels(dev, tmp_path):
    from dynamicvectorquantization_amd import evaluate as E
    root = _folder(tmp_path)
    a = torch.cat(list(E.image_batches(3, 64, dev, root)))
    b = torch.cat(list(E.image_batches(3, 64, dev, root, device_png=True)))
    c = torch.cat(list(E.image_batches(3, 64, dev, root, device_decode=True, device_png=True)))
    assert a.shape == (8, 3, 64, 64) and torch.equal(a, b) and torch.equal(a, c)


def _ffhq_tree(root, n=8, size=96):
    (root / "FFHQ").mkdir(parents=True)
    (root / "assets").mkdir()
    names = [f"{i:05d}.png" for i in range(n)]
    pix = {}
    for i, name in enumerate(names):
        pix[name] = pm.picture(size + (i % 3), size + (i % 3), 3, 70 + i)
        (root / "FFHQ" / name).write_bytes(pm.write_png(pix[name], np.random.default_rng(i).integers(0, 5, size=pix[name].shape[0])))
    (root / "assets" / "ffhqtrain.txt").write_text("".join(f"{n}\n" for n in names))
    (root / "assets" / "ffhqvalidation.txt").write_text("".join(f"{n}\n" for n in names[:4]))
    return names, pix


def test_ffhq_train_transform_equals_pil_crop_resize_flip(dev, tmp_path, monkeypatch):
    """FFHQ(split="train") through GpuBatchLoader with injected boxes (the sampler is replaced; the flips are the loader's own draws, which
    the test repeats from the same seed) == crop, resize, flip, normalise with PIL and numpy on the host, bit for bit"""
    from PIL import Image
    names, pix = _ffhq_tree(tmp_path)
    S = 32
    rs = np.random.RandomState(4)
    boxes = []
    for name in names:
        side = pix[name].shape[0]
        bs = int(rs.randint(int(side * 0.86), side + 1))
        boxes.append((int(rs.randint(0, side - bs + 1)), int(rs.randint(0, side - bs + 1)), bs, bs))
    boxes[0] = (0, 0, pix[names[0]].shape[1], pix[names[0]].shape[0])          # the whole image
    for device_png in (False, True):
        queue = list(boxes)
        monkeypatch.setattr(D, "sample_square_box", lambda w, h, rng, scale=None: queue.pop(0))
        ds = D.FFHQ(split="train", root=str(tmp_path))
        loader = D.GpuBatchLoader(ds, 4, dev, size=S, shuffle=False, num_workers=2, seed=11, device_png=device_png)
        flips = np.random.default_rng(11)
        seen = 0
        for b in loader:
            assert set(b) == {"image", "file_path_"} and tuple(b["image"].shape) == (4, 3, S, S)
            got = b["image"].cpu().numpy()
            for k in range(4):
                name = os.path.basename(b["file_path_"][k])
                left, top, bw, bh = boxes[names.index(name)]
                ref = np.asarray(Image.fromarray(pix[name], "RGB").crop((left, top, left + bw, top + bh)).resize((S, S), Image.BILINEAR))
                flip = bool(flips.random() < 0.5)
                assert np.array_equal(got[k], odata.finish(ref, S, 0, 0, flip)), f"{name} device_png={device_png}"
                seen += 1
        assert seen == 8 and not queue
    # the validation split gets the eval transform (Resize + CenterCrop), as every dataset does
    va = D.GpuBatchLoader(D.FFHQ(split="val", root=str(tmp_path)), 4, dev, size=S, num_workers=2, device_png=True)
    (b,) = list(va)
    for k in range(4):
        assert np.array_equal(b["image"][k].cpu().numpy(), odata.reference_transform(pix[names[k]], S))


def test_train_py_ffhq_config_device_png(dev, tmp_path):
    """`train.py --base configs/stage1/dqvae-entropy-dual-r05_ffhq.yml --real_data --device_png`: two steps on a tiny generated tree, the
    model shrunk as in the other train.py tests (a second base file overrides the model section; the router keeps the FFHQ thresholds)"""
    import yaml
    from conftest import REPO
    from test_gpu_model import GEOM, model_config
    _ffhq_tree(tmp_path / "ffhq", n=8, size=70)
    mc = model_config(**GEOM["small"], loss="ae")
    mc["base_learning_rate"] = 1e-5
    mc["params"]["encoderconfig"]["params"]["router_config"]["params"].pop("json_path")
    small = tmp_path / "small.yml"
    yaml.safe_dump({"model": mc}, open(small, "w"))
    logs = tmp_path / "logs"
    root = str(tmp_path / "ffhq")
    cmd = [sys.executable, os.path.join(REPO, "train.py"), "--base", os.path.join(REPO, "configs", "stage1", "dqvae-entropy-dual-r05_ffhq.yml"),
           str(small), "--real_data", "--device_png", "--max_epochs", "1", "--max_steps", "2", "--check_val_every_n_epoch", "0",
           "--logdir", str(logs), "-n", "f", f"data.params.train.params.root={root}", f"data.params.validation.params.root={root}",
           "data.params.batch_size=4", "data.params.num_workers=2"]
    r = subprocess.run(cmd, cwd=REPO, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert "device PNG decode" in r.stdout
    run = os.listdir(logs)
    ck = torch.load(logs / run[0] / "checkpoints" / "last.ckpt", map_location="cpu", weights_only=False)
    assert ck["global_step"] == 2
    saved = yaml.safe_load(open(logs / run[0] / "configs" / "project.yaml"))
    assert saved["data"]["params"]["train"]["target"] == "data.faceshq.FFHQ"
    assert saved["model"]["params"]["encoderconfig"]["params"]["router_config"]["params"]["json_path"].endswith("ffhq_train_patch-16.json")
    # without --real_data the flag is an error, before any model is built
    r = subprocess.run([sys.executable, os.path.join(REPO, "train.py"), "-b", str(small), "--device_png", "--logdir", str(logs)],
                       cwd=REPO, capture_output=True, text=True, timeout=600)
    assert r.returncode != 0 and "--device_png needs --real_data" in r.stderr
