"""Host-side tests of the likelihood evaluation (docs/design/15-likelihood.md): the numpy aggregation of per-image stream sums in
dynamicvectorquantization_amd.evaluate and the command line of scripts/tools/eval_likelihood.py."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from dynamicvectorquantization_amd import evaluate as E

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCRIPT = os.path.join(REPO, "scripts", "tools", "eval_likelihood.py")


def hand_made():
    """three images; columns: nll sum (nats), tokens, top-1 hits, top-5 hits; rows: content coarse / fine, position coarse / fine"""
    a = np.zeros((3, 4, 4), dtype=np.float64)
    a[0] = [[12.0, 4, 1, 3], [30.0, 10, 2, 5], [6.0, 4, 2, 4], [20.0, 10, 0, 1]]
    a[1] = [[9.0, 3, 0, 1], [0.0, 0, 0, 0], [3.0, 3, 3, 3], [0.5, 1, 1, 1]]           # no fine content: only the fine <eos> position
    a[2] = [[15.0, 5, 5, 5], [48.0, 16, 4, 8], [5.0, 5, 1, 2], [32.0, 16, 3, 9]]
    return a


def test_streams_perplexity_accuracy_and_token_counts():
    a = hand_made()
    s = E.aggregate_likelihood(a)
    assert s["n_images"] == 3 and tuple(s["streams"]) == E.LIKELIHOOD_STREAMS
    for i, name in enumerate(E.LIKELIHOOD_STREAMS):
        st = s["streams"][name]
        total, count = a[:, i, 0].sum(), a[:, i, 1].sum()
        assert st["tokens"] == int(count)
        assert st["nats_per_token"] == pytest.approx(total / count, rel=1e-15)
        assert st["perplexity"] == pytest.approx(math.exp(total / count), rel=1e-14)
        assert st["top1"] == pytest.approx(a[:, i, 2].sum() / count, rel=1e-15)
        assert st["top5"] == pytest.approx(a[:, i, 3].sum() / count, rel=1e-15)
        assert st["tokens_per_image"] == {"mean": pytest.approx(a[:, i, 1].mean()), "min": int(a[:, i, 1].min()), "max": int(a[:, i, 1].max())}
    assert s["streams"]["content_fine"]["tokens_per_image"]["min"] == 0
    assert s["tokens_per_image"] == {"mean": pytest.approx((28 + 7 + 42) / 3), "min": 7, "max": 42}


def test_empty_stream_gives_none_not_nan():
    a = hand_made()
    a[:, 1] = 0.0                                            # nobody has a fine content token
    s = E.aggregate_likelihood(a, pixels_per_image=12)
    st = s["streams"]["content_fine"]
    assert st["nats_per_token"] is None and st["perplexity"] is None and st["top1"] is None and st["top5"] is None and st["tokens"] == 0
    assert st["tokens_per_image"] == {"mean": 0.0, "min": 0, "max": 0}
    assert s["loss"]["content_loss"] == pytest.approx(36.0 / 12)       # the coarse content tokens alone
    a[:, 3] = 0.0                                            # no fine position target either: that loss, and what is built on it, is None
    s = E.aggregate_likelihood(a)
    assert s["loss"]["fine_position_loss"] is None and s["loss"]["position_loss"] is None and s["loss"]["loss"] is None
    assert s["loss"]["coarse_position_loss"] == pytest.approx(14.0 / 12)
    text = __import__("json").dumps(s)
    assert "NaN" not in text and "Infinity" not in text
    empty = E.aggregate_likelihood(np.zeros((0, 4, 4)))
    assert empty["n_images"] == 0 and empty["nats_per_image"] is None and empty["bits_per_pixel"] is None


def test_bits_per_image_and_per_pixel():
    a = hand_made()
    s = E.aggregate_likelihood(a, pixels_per_image=64 * 64 * 3)
    nats = a[:, :, 0].sum() / 3
    assert s["nats_per_image"] == pytest.approx(nats, rel=1e-15)
    assert s["bits_per_image"] == pytest.approx(nats / math.log(2.0), rel=1e-15)
    assert s["bits_per_pixel"] == pytest.approx(nats / math.log(2.0) / 12288, rel=1e-15) and s["pixels_per_image"] == 12288
    assert E.aggregate_likelihood(a)["bits_per_pixel"] is None
    one = np.zeros((1, 4, 4))
    one[0, 0] = [math.log(2.0) * 24, 3, 0, 0]               # 24 bits over 2 x 2 x 3 values
    assert E.aggregate_likelihood(one, pixels_per_image=12)["bits_per_pixel"] == pytest.approx(2.0, rel=1e-15)


def test_weighted_loss_is_the_training_steps():
    """Dualformer._step: content = CE over all content targets of the batch, position = (coarse + fine) / 2, total = wc * content +
    wp * position"""
    a = hand_made()
    s = E.aggregate_likelihood(a, content_loss_weight=1.0, position_loss_weight=0.7, batch_sizes=[2, 1])
    content = (12 + 30 + 9 + 0 + 15 + 48) / (4 + 10 + 3 + 0 + 5 + 16)
    coarse, fine = (6 + 3 + 5) / 12, (20 + 0.5 + 32) / 27
    assert s["loss"]["content_loss"] == pytest.approx(content, rel=1e-15)
    assert s["loss"]["coarse_position_loss"] == pytest.approx(coarse, rel=1e-15)
    assert s["loss"]["fine_position_loss"] == pytest.approx(fine, rel=1e-15)
    assert s["loss"]["position_loss"] == pytest.approx((coarse + fine) / 2, rel=1e-15)
    assert s["loss"]["loss"] == pytest.approx(content + 0.7 * (coarse + fine) / 2, rel=1e-15)
    assert s["content_loss_weight"] == 1.0 and s["position_loss_weight"] == 0.7
    # per batch, then the mean over batches (an epoch average of the logged validation losses)
    b0 = E.step_losses(a[:2].sum(axis=0), 1.0, 0.7)
    b1 = E.step_losses(a[2], 1.0, 0.7)
    assert b0["content_loss"] == pytest.approx((12 + 30 + 9) / 17) and b0["fine_position_loss"] == pytest.approx(20.5 / 11)
    assert b1["loss"] == pytest.approx(63 / 21 + 0.7 * (1.0 + 2.0) / 2)
    for k in ("content_loss", "position_loss", "coarse_position_loss", "fine_position_loss", "loss"):
        assert s["loss_batch_mean"][k] == pytest.approx((b0[k] + b1[k]) / 2, rel=1e-15)
    assert E.aggregate_likelihood(a)["loss_batch_mean"] is None
    with pytest.raises(ValueError):
        E.aggregate_likelihood(a, batch_sizes=[2, 2])
    with pytest.raises(ValueError):
        E.aggregate_likelihood(np.zeros((3, 4, 3)))


def test_read_labels(tmp_path):
    np.save(tmp_path / "l.npy", np.array([3, 0, 9], dtype=np.int32))
    assert E.read_labels(str(tmp_path / "l.npy")).tolist() == [3, 0, 9] and E.read_labels(str(tmp_path / "l.npy")).dtype == np.int64
    (tmp_path / "l.txt").write_text("1, 2\n7\n")
    assert E.read_labels(str(tmp_path / "l.txt")).tolist() == [1, 2, 7]
    np.save(tmp_path / "bad.npy", np.zeros((2, 2)))
    with pytest.raises(ValueError):
        E.read_labels(str(tmp_path / "bad.npy"))


def test_script_help_and_argument_errors(tmp_path):
    r = subprocess.run([sys.executable, SCRIPT, "--help"], capture_output=True, text=True, timeout=120, cwd=REPO)
    assert r.returncode == 0, r.stderr[-2000:]
    for flag in ("--yaml_path", "--model_path", "--batch_size", "--dataset_type", "--images", "--synthetic", "--limit", "--dtype",
                 "--labels", "--json", "--per_image"):
        assert flag in r.stdout, flag
    base = [sys.executable, SCRIPT, "--yaml_path", "configs/stage2/uncond_imagenet_p6c18.yml"]
    # every argument error exits with 2 before any model or device work
    r = subprocess.run(base + ["--dataset_type", "ffhq"], capture_output=True, text=True, timeout=120, cwd=REPO)
    assert r.returncode == 2 and "--images" in r.stderr, r.stderr[-2000:]
    r = subprocess.run(base + ["--synthetic", "2", "--per_image", str(tmp_path / "x.txt")], capture_output=True, text=True, timeout=120,
                       cwd=REPO)
    assert r.returncode == 2 and ".npy" in r.stderr, r.stderr[-2000:]
    r = subprocess.run(base + ["--synthetic", "2", "--labels", str(tmp_path / "missing.txt")], capture_output=True, text=True,
                       timeout=120, cwd=REPO)
    assert r.returncode == 2 and "--labels" in r.stderr, r.stderr[-2000:]


def test_script_parser_defaults():
    sys.path.insert(0, os.path.dirname(SCRIPT))
    try:
        import eval_likelihood
    finally:
        sys.path.pop(0)
    opt = eval_likelihood.get_parser().parse_args(["--yaml_path", "y.yml", "--synthetic", "4", "--batch_size", "2", "--per_image", "p.npy"])
    assert (opt.yaml_path, opt.synthetic, opt.batch_size, opt.per_image, opt.labels, opt.json, opt.dtype) == ("y.yml", 4, 2, "p.npy", "", "", "bf16")
