"""Host side of deterministic training (docs/design/21-reproducible-training.md): the command-line flag, the Trainer argument and the
library's counter of unordered launches.  No GPU needed."""
import inspect
import os
import sys

from conftest import REPO


def _train():
    sys.path.insert(0, REPO)
    import train
    return train


def test_train_py_deterministic_flag_parses_and_defaults_off():
    train = _train()
    p = train.get_parser()
    opt, unknown = p.parse_known_args(["-b", "configs/stage1/dqvae-entropy-dual-r05_imagenet.yml"])
    assert opt.deterministic is False and unknown == []
    opt, unknown = p.parse_known_args(["-b", "x.yml", "--deterministic", "--benchmark", "True", "model.params.image_size=64"])
    assert opt.deterministic is True
    dot, ignored = train.split_unknown(unknown)
    assert dot == ["model.params.image_size=64"]
    assert ignored == ["--benchmark", "True"] and "--deterministic" not in ignored


def test_deterministic_flag_round_trips_through_the_saved_config():
    """train.py stores the flag as lightning.trainer.deterministic of the run's project.yaml; a resumed run reads it back from there"""
    from dynamicvectorquantization_amd import config as cfg
    base = cfg.load_yaml(os.path.join(REPO, "configs/stage1/dqvae-entropy-dual-r05_imagenet.yml"))
    assert not base.get("lightning", {}).get("trainer", {}).get("deterministic", False)
    merged = cfg.merge(base, cfg.from_dotlist(["lightning.trainer.deterministic=true"]))
    plain = cfg.to_plain(merged)
    assert plain["lightning"]["trainer"]["deterministic"] is True and plain["model"] == cfg.to_plain(base)["model"]
    src = open(os.path.join(REPO, "train.py")).read()
    assert "lightning.trainer.deterministic=true" in src and "deterministic=deterministic" in src


def test_trainer_signature_carries_deterministic_false():
    from dynamicvectorquantization_amd.trainer import Trainer
    par = inspect.signature(Trainer.__init__).parameters
    assert "deterministic" in par and par["deterministic"].default is False


def test_library_exports_the_unordered_launch_counter():
    from dynamicvectorquantization_amd import _lib, build
    from dynamicvectorquantization_amd import kernels as K
    build.build(verbose=False)
    lib = _lib.load()
    assert "dvq_unordered_launches" in _lib.SIGNATURES and hasattr(lib, "dvq_unordered_launches")
    header = open(os.path.join(REPO, "include", "dvq_hip.h")).read()
    assert "long long dvq_unordered_launches(void);" in header
    assert lib.dvq_version() >= 118
    n = K.unordered_launches()
    assert isinstance(n, int) and n >= 0 and K.unordered_launches() == n          # nothing was launched in between


def test_reseed_draws_restarts_the_dropout_seed_sequence():
    import torch
    from dynamicvectorquantization_amd import runtime as rt
    torch.manual_seed(5)
    rt.reseed_draws()
    a = [rt.next_dropout_seed() for _ in range(3)]
    rt.next_dropout_seed()
    rt.reseed_draws()
    assert [rt.next_dropout_seed() for _ in range(3)] == a and len(set(a)) == 3
