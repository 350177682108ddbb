"""Weight EMA, the parts that need no GPU (docs/design/20-weight-ema.md): the decay schedule, evaluate.checkpoint_state_dict,
scripts/tools/export_ema.py on a hand-made checkpoint, train.py's flags."""
import os
import subprocess
import sys

import pytest
import torch

import train
from dynamicvectorquantization_amd import evaluate as E
from dynamicvectorquantization_amd.trainer import ema_decay_at

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPORT = os.path.join(REPO, "scripts", "tools", "export_ema.py")


# ---- schedule -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 9, 10, 10 ** 6])
def test_decay_schedule_closed_form(n):
    for decay in (0.5, 0.999, 0.9999):
        assert ema_decay_at(n, decay, True) == min(decay, (1 + n) / (10 + n))
        assert ema_decay_at(n, decay, False) == decay
    assert ema_decay_at(n, 0.9999) == ema_decay_at(n, 0.9999, True)           # warm-up is the default


def test_decay_schedule_examples():
    assert ema_decay_at(1, 0.9999, True) == 2 / 11
    assert ema_decay_at(2, 0.9999, True) == 3 / 12
    assert ema_decay_at(9, 0.9999, True) == 10 / 19
    assert ema_decay_at(10, 0.5, True) == 0.5                                  # 11 / 20 > 0.5: the cap
    # (1 + n) / (10 + n) >= 0.9999  <=>  n >= 89990: the cap is reached there, exactly, and not one update earlier
    assert (1 + 89990) / (10 + 89990) >= 0.9999 > (1 + 89989) / (10 + 89989)
    assert ema_decay_at(89989, 0.9999, True) < 0.9999
    assert ema_decay_at(89990, 0.9999, True) == 0.9999
    assert ema_decay_at(10 ** 6, 0.9999, True) == 0.9999
    ds = [ema_decay_at(n, 0.9999, True) for n in range(1, 200)]
    assert all(a < b for a, b in zip(ds, ds[1:]))                              # strictly rising during the warm-up


# ---- checkpoint_state_dict -------------------------------------------------------------------------------------------------------
def _checkpoint():
    g = torch.Generator().manual_seed(3)
    sd = {"conv.weight": torch.randn(4, 3, 3, 3, generator=g), "conv.bias": torch.randn(4, generator=g),
          "head.weight": torch.randn(5, 4, generator=g), "bn.running_mean": torch.randn(4, generator=g),
          "quantize.embedding.weight": torch.randn(8, 4, generator=g)}
    ema = {"conv.weight": torch.randn(4, 3, 3, 3, generator=g), "conv.bias": torch.randn(4, generator=g),
           "head.weight": torch.randn(5, 4, generator=g)}
    return {"state_dict": sd, "global_step": 40, "epoch": 3,
            "optimizer_states": [{"state": {0: {"step": torch.tensor(40.0), "exp_avg": torch.zeros(4)}}, "param_groups": []}],
            "lr_schedulers": [{"last_epoch": 40}],
            "ema": {"decay": 0.999, "warmup": True, "num_updates": 40, "state_dict": ema}}


def test_checkpoint_state_dict_plain_forms():
    ckpt = _checkpoint()
    assert E.checkpoint_state_dict(ckpt) is ckpt["state_dict"]
    assert E.checkpoint_state_dict(ckpt, use_ema=False) is ckpt["state_dict"]
    bare = ckpt["state_dict"]
    assert E.checkpoint_state_dict(bare) is bare


def test_checkpoint_state_dict_overlay():
    ckpt = _checkpoint()
    before = {k: v.clone() for k, v in ckpt["state_dict"].items()}
    out = E.checkpoint_state_dict(ckpt, use_ema=True)
    assert out is not ckpt["state_dict"] and list(out) == list(ckpt["state_dict"])
    for k in out:
        if k in ckpt["ema"]["state_dict"]:
            assert torch.equal(out[k], ckpt["ema"]["state_dict"][k]) and not torch.equal(out[k], before[k]), k
        else:                                                                  # buffers, the forward-updated codebook: untouched
            assert out[k] is ckpt["state_dict"][k], k
    assert sorted(k for k in out if out[k] is not ckpt["state_dict"][k]) == sorted(ckpt["ema"]["state_dict"])
    for k, v in before.items():                                                # the input is not modified
        assert torch.equal(ckpt["state_dict"][k], v), k
    assert set(ckpt) == {"state_dict", "global_step", "epoch", "optimizer_states", "lr_schedulers", "ema"}


def test_checkpoint_state_dict_errors():
    ckpt = _checkpoint()
    no_ema = {k: v for k, v in ckpt.items() if k != "ema"}
    with pytest.raises(KeyError, match="ema"):
        E.checkpoint_state_dict(no_ema, use_ema=True)
    with pytest.raises(KeyError, match="ema"):
        E.checkpoint_state_dict(ckpt["state_dict"], use_ema=True)              # a bare state dict has no averaged weights
    unknown = _checkpoint()
    unknown["ema"]["state_dict"]["tail.weight"] = torch.zeros(2)
    with pytest.raises(KeyError, match="tail.weight"):
        E.checkpoint_state_dict(unknown, use_ema=True)
    shape = _checkpoint()
    shape["ema"]["state_dict"]["conv.bias"] = torch.zeros(5)
    with pytest.raises(KeyError, match="conv.bias"):
        E.checkpoint_state_dict(shape, use_ema=True)


# ---- export_ema.py -------------------------------------------------------------------------------------------------------------
def _run_export(src, dst):
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="")     # CPU only
    return subprocess.run([sys.executable, EXPORT, "--in", str(src), "--out", str(dst)], capture_output=True, text=True, env=env)


def test_export_ema(tmp_path):
    ckpt = _checkpoint()
    src, dst, again = tmp_path / "a.ckpt", tmp_path / "b.ckpt", tmp_path / "c.ckpt"
    torch.save(ckpt, src)
    r = _run_export(src, dst)
    assert r.returncode == 0, r.stderr
    out = torch.load(dst, map_location="cpu")
    want = E.checkpoint_state_dict(ckpt, use_ema=True)
    assert list(out["state_dict"]) == list(want)
    for k in want:
        assert torch.equal(out["state_dict"][k], want[k]), k
    assert out["global_step"] == 40 and out["epoch"] == 3
    assert "optimizer_states" not in out and "lr_schedulers" not in out and "ema" not in out
    assert out["ema_exported"] == {"decay": 0.999, "num_updates": 40}
    r = _run_export(dst, again)                                                # the output holds no "ema" key: nothing to export
    assert r.returncode != 0 and "ema" in r.stderr and not again.exists()


# ---- train.py ------------------------------------------------------------------------------------------------------------------
def test_parser_takes_the_flags_and_defaults_are_off():
    opt, unknown = train.get_parser().parse_known_args(["-b", "x.yml"])
    assert opt.ema_decay == 0.0 and opt.ema_no_warmup is False and unknown == []
    opt, unknown = train.get_parser().parse_known_args(["-b", "x.yml", "--ema_decay", "0.999", "--ema_no_warmup"])
    assert opt.ema_decay == 0.999 and opt.ema_no_warmup is True and unknown == []


def test_flags_are_not_in_the_ignored_list():
    argv = ["-b", "x.yml", "--ema_decay", "0.999", "--ema_no_warmup", "--accumulate_grad_batches", "2"]
    _, unknown = train.get_parser().parse_known_args(argv)
    dot, ignored = train.split_unknown(unknown)
    assert dot == [] and ignored == ["--accumulate_grad_batches", "2"]
