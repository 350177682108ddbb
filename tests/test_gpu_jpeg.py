"""GPU tests of the device JPEG decode (docs/design/23-device-jpeg.md): dvq_jpeg_batch_decode against the numpy restatement of its
arithmetic (tests/jpeg_math.py) and against PIL, byte for byte; the loader with device_decode against the loader without; train.py
--device_jpeg.  Exact equality everywhere: the arithmetic is integer."""
import io
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import jpeg_math as jm
from dynamicvectorquantization_amd import data as D

pytestmark = pytest.mark.gpu


def test_batch_decode_equals_restatement_and_pil(dev):
    """the whole case matrix in ONE launch pair, sizes mixed (offsets, items that end inside a workgroup, a 500 x 375 image whose grids
    span several workgroups), with a host-decoded image between them whose slot the kernels must leave alone"""
    from PIL import features
    names = [c[0] for c in jm.CASES]
    names = names[-1:] + names[:-1]                      # the large image first: everything after it sits at large offsets
    datas = [jm.case_bytes(n) for n in names]
    records = [D.decode_jpeg_host(d) for d in datas]
    assert all(r is not None for r in records)
    extra = jm.test_image(21, 13, "RGB", 99)
    records.insert(3, extra)
    out = D.decode_batch_gpu(records, dev)
    torch.cuda.synchronize()
    rgb = out["rgb"].cpu().numpy()
    got = [rgb[o:o + h * w * 3].reshape(h, w, 3) for o, (w, h) in zip(out["offs"], out["sizes"])]
    assert all(o % 16 == 0 for o in out["offs"])
    assert np.array_equal(got.pop(3), extra)
    for name, data, g in zip(names, datas, got):
        ref = jm.decode(data)
        assert g.shape == ref.shape and np.array_equal(g, ref), f"{name}: {(g != ref).sum()} bytes differ from the restatement"
        if features.check_feature("libjpeg_turbo"):
            assert np.array_equal(g, jm.pil_rgb(data)), f"{name}: differs from PIL"


def _folder(tmp_path, split="val", big=True):
    """<tmp>/<split>/<class>/...: supported JPEGs of every sampling, one progressive JPEG, one PNG"""
    from PIL import Image
    specs = [("n01", "a.jpg", 90, 70, dict(quality=90, subsampling=2)), ("n01", "b.jpg", 64, 100, dict(quality=75, subsampling=1)),
             ("n01", "c.jpg", 81, 67, dict(quality=95, subsampling=0)), ("n01", "d.jpg", 70, 70, dict(quality=85, progressive=True)),
             ("n02", "e.png", 75, 66, None), ("n02", "f.jpg", 77, 93, dict(quality=80, subsampling=2, restart_marker_blocks=2)),
             ("n02", "g.jpg", 66, 65, dict(quality=60)), ("n02", "h.jpg", 120 if big else 68, 71, dict(quality=92, subsampling=2))]
    for i, (c, f, w, h, opts) in enumerate(specs):
        d = tmp_path / split / c
        d.mkdir(parents=True, exist_ok=True)
        im = jm.test_image(w, h, "L" if f == "g.jpg" else "RGB", 40 + i)
        Image.fromarray(im, "L" if f == "g.jpg" else "RGB").save(d / f, "PNG" if opts is None else "JPEG", **(opts or {}))
    return str(tmp_path / split)


def test_loader_parity_eval_and_train(dev, tmp_path):
    root = _folder(tmp_path)
    kinds = [set(D.ImageFolder(root, device_decode=True)[i]) & {"jpeg", "image_u8"} for i in range(8)]
    assert kinds == [{"jpeg"}] * 3 + [{"image_u8"}] * 2 + [{"jpeg"}] * 3          # the progressive file and the PNG stay with PIL

    def batches(device_decode, train, seed=3):
        ds = D.ImageFolder(root, is_train=train)
        loader = D.GpuBatchLoader(ds, 4, dev, size=64, shuffle=train, num_workers=2, seed=seed, device_decode=device_decode)
        return [{k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in b.items()} for b in loader]
    for train in (False, True):
        a, b = batches(False, train), batches(True, train)
        assert len(a) == len(b) == 2
        for x, y in zip(a, b):
            assert set(x) == set(y) and x["image"].shape == (4, 3, 64, 64)
            assert np.array_equal(x["image"], y["image"]), f"train={train}: {(x['image'] != y['image']).sum()} elements differ"
            assert np.array_equal(x["class_label"], y["class_label"]) and list(x["relpath"]) == list(y["relpath"])
    # injected crops and flips, through the planning siblings
    ds_off, ds_on = D.ImageFolder(root), D.ImageFolder(root, device_decode=True)
    ims = [ds_off[i]["image_u8"] for i in range(8)]
    rs = np.random.RandomState(1)
    crops, flips = [], []
    for im in ims:
        nw, nh = D.resized_size(im.shape[1], im.shape[0], 64)
        crops.append((int(rs.randint(0, nw - 64 + 1)), int(rs.randint(0, nh - 64 + 1))))
        flips.append(bool(rs.randint(0, 2)))
    ref = D.transform_batch_gpu(D.plan_batch(ims, 64, crops=crops, flips=flips), dev)
    ex = [ds_on[i] for i in range(8)]
    dec = D.decode_batch_gpu([e["jpeg"] if "jpeg" in e else e["image_u8"] for e in ex], dev)
    got = D.transform_batch_device(D.plan_batch_sizes(dec["sizes"], 64, crops=crops, flips=flips, src_offs=dec["offs"]), dec["rgb"], dev)
    assert torch.equal(ref, got)


def test_tools_see_the_same_pixels(dev, tmp_path):
    """what the forward-only tools read: evaluate.image_batches (eval_reconstruction, codebook_usage_dqvae, calculate_entropy_thresholds)
    and the tokeniser's view batches (center, flip, random crops) are bit-identical with and without device_decode"""
    import importlib.util

    from conftest import REPO
    from dynamicvectorquantization_amd import evaluate as E
    root = _folder(tmp_path)
    a = torch.cat(list(E.image_batches(3, 64, dev, root)))
    b = torch.cat(list(E.image_batches(3, 64, dev, root, device_decode=True)))
    assert a.shape == (8, 3, 64, 64) and torch.equal(a, b)
    spec = importlib.util.spec_from_file_location("dvq_tokenize_dataset", os.path.join(REPO, "scripts", "tools", "tokenize_dataset.py"))
    tok = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tok)
    views = ["center", "flip", "random:0", "random:1"]
    ds = E.folder_dataset(root)
    off = list(tok.decoded_view_batches(ds, views, 1, 8, 4, 64, dev, 7, 2))
    on = list(tok.decoded_view_batches(ds, views, 1, 8, 4, 64, dev, 7, 2, device_decode=True))
    assert len(off) == len(on) == 2
    for (xa, la, ia), (xb, lb, ib) in zip(off, on):
        assert np.array_equal(la, lb) and np.array_equal(ia, ib) and len(xa) == len(xb) == 4
        assert all(torch.equal(u, v) for u, v in zip(xa, xb))
    assert not torch.equal(off[0][0][0], off[0][0][1])          # the views differ from each other


def test_train_py_device_jpeg(dev, tmp_path):
    """`train.py --real_data --device_jpeg`: two steps on a tiny folder of JPEG files"""
    import yaml
    from conftest import REPO
    from test_gpu_model import GEOM, model_config
    for split in ("train", "val"):
        _folder(tmp_path / "imgs", split, big=False)
    mc = model_config(**GEOM["small"], loss="ae")
    mc["base_learning_rate"] = 1e-5
    cfg_path = tmp_path / "tiny.yml"
    yaml.safe_dump({"model": mc, "data": {"target": "data.build.DataModuleFromConfig", "params": {
        "batch_size": 4, "num_workers": 2,
        "train": {"target": "data.imagenet.ImageNetTrain", "params": {"config": {"is_eval": False, "size": 64}}},
        "validation": {"target": "data.imagenet.ImageNetValidation", "params": {"config": {"is_eval": True, "size": 64}}}}}},
        open(cfg_path, "w"))
    env = dict(os.environ, DVQ_IMAGENET_ROOT=str(tmp_path / "imgs"))
    logs = tmp_path / "logs"
    cmd = [sys.executable, os.path.join(REPO, "train.py"), "-b", str(cfg_path), "--real_data", "--device_jpeg", "--max_epochs", "1", "--max_steps", "2",
           "--check_val_every_n_epoch", "0", "--logdir", str(logs), "-n", "j"]
    r = subprocess.run(cmd, env=env, cwd=REPO, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert "device JPEG decode" in r.stdout
    run = os.listdir(logs)
    ck = torch.load(logs / run[0] / "checkpoints" / "last.ckpt", map_location="cpu", weights_only=False)
    assert ck["global_step"] == 2
    # without --real_data the flag is an error, before any model is built
    r = subprocess.run([sys.executable, os.path.join(REPO, "train.py"), "-b", str(cfg_path), "--device_jpeg", "--logdir", str(logs)],
                       env=env, cwd=REPO, capture_output=True, text=True, timeout=600)
    assert r.returncode != 0 and "--device_jpeg needs --real_data" in r.stderr
