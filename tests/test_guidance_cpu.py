"""Host-side tests of classifier-free guidance (docs/design/14-guidance.md): the class-conditional sampling script's --classes parser
and npz writer, the null-label table check as a function of the config, and the op-by-op guided draw (pure torch)."""
import importlib
import os
import sys

import numpy as np
import pytest
import torch

from dynamicvectorquantization_amd import config as cfg
from dynamicvectorquantization_amd import stage2

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _script():
    sys.path.insert(0, os.path.join(REPO, "scripts", "sample_val"))
    try:
        return importlib.import_module("sample_dynamic_class")
    finally:
        sys.path.pop(0)


def test_classes_parser():
    s = _script()
    assert s.parse_classes("", 5) == [0, 1, 2, 3, 4]
    assert s.parse_classes("0-999", 1000) == list(range(1000))
    assert s.parse_classes("0,3,7", 10) == [0, 3, 7]
    assert s.parse_classes("7, 3,0", 10) == [7, 3, 0]                     # the given order is the output order
    assert s.parse_classes("2-4,9", 10) == [2, 3, 4, 9]
    assert s.parse_classes("5", 10) == [5]
    for bad in ("10", "3-1", "0-10", ",", "a"):
        with pytest.raises(ValueError):
            s.parse_classes(bad, 10)


def test_script_defaults():
    opt = _script().get_parser().parse_args([])
    assert (opt.batch_size, opt.per_class, opt.cfg_scale, opt.npz, opt.classes) == (32, 50, 1.0, False, "")
    assert opt.top_k == 300 and opt.streams == 4                          # the unconditional script's flags are inherited


def test_npz_layout(tmp_path):
    s = _script()
    rng = np.random.default_rng(0)
    img = rng.random((6, 3, 4, 5), dtype=np.float32)
    img[0, 0, 0, 0], img[0, 0, 0, 1] = 0.0, 1.0
    u8 = s.to_uint8_nhwc(img)
    assert u8.dtype == np.uint8 and u8.shape == (6, 4, 5, 3)
    assert u8[0, 0, 0, 0] == 0 and u8[0, 0, 1, 0] == 255
    np.testing.assert_array_equal(u8, np.floor(img.transpose(0, 2, 3, 1) * 255.0 + 0.5).astype(np.uint8))
    labels = np.array([0, 0, 3, 3, 7, 7])
    path = s.write_npz(str(tmp_path), u8, labels)
    assert os.path.basename(path) == "samples_6x4x5x3.npz"
    with np.load(path) as f:
        assert sorted(f.files) == ["arr_0", "arr_1"]
        assert f["arr_0"].dtype == np.uint8 and np.array_equal(f["arr_0"], u8)
        assert f["arr_1"].dtype == np.int64 and f["arr_1"].tolist() == [0, 0, 3, 3, 7, 7]
    with pytest.raises(AssertionError):
        s.write_npz(str(tmp_path), u8, labels[:5])


def _class_params(path):
    p = cfg.load_yaml(os.path.join(REPO, path)).model["params"]
    return p["transformer_config"]["params"], p["class_cond_stage_config"]["params"]


def test_null_label_table_check():
    gpt = dict(vocab_size=525, coarse_position_size=29, fine_position_size=77)
    prov = dict(n_classes=10, threshold_content=514, threshold_coarse_position=18, threshold_fine_position=66, fine_seg_sos=1)
    assert stage2.null_label_table_errors(gpt, prov) == []
    # one table at a time without its null row (null label = n_classes: id threshold + n_classes must be < size)
    for table in gpt:
        errs = stage2.null_label_table_errors(dict(gpt, **{table: gpt[table] - 1}), prov)
        assert len(errs) == 1 and errs[0].startswith(table) and str(gpt[table]) in errs[0], errs
    # no fine start tokens: the fine-position table is not checked
    assert stage2.null_label_table_errors(dict(gpt, fine_position_size=1), dict(prov, fine_seg_sos=None)) == []
    # the shipped configs: the reference's sizes have no null row in any table, the _cfg config has one in each
    errs = stage2.null_label_table_errors(*_class_params("configs/stage2/class_imagenet_p6c18.yml"))
    assert [e.split(" ")[0] for e in errs] == ["vocab_size", "coarse_position_size", "fine_position_size"]
    assert stage2.null_label_table_errors(*_class_params("configs/stage2/class_imagenet_p6c18_cfg.yml")) == []
    m = cfg.load_yaml(os.path.join(REPO, "configs/stage2/class_imagenet_p6c18_cfg.yml")).model
    assert m["params"]["cond_drop_prob"] == 0.1
    assert cfg.load_yaml(os.path.join(REPO, "configs/stage2/class_imagenet_p6c18.yml")).model["params"].get("cond_drop_prob") is None


def test_op_by_op_guided_draw():
    """_draw(cfg=s) on [c ; u] rows: s = 1 draws from c, s = 0 from u, any s greedily the argmax of (1 - s) u + s c under the rule;
    the pair's token comes back in both halves"""
    g = torch.Generator().manual_seed(3)
    b, v = 5, 40
    lg = torch.randn(2 * b, 1, v, generator=g) * 3
    c, u = lg[:b, -1], lg[b:, -1]

    def rule(x):                                  # a 2B-row rule: forbid column 0 everywhere, column 1 on the second half only
        x = x.clone()
        x[:, 0] = -float("inf")
        x[x.shape[0] // 2:, 1] = -float("inf")
        return x

    draw = stage2._SamplerMixin._draw
    for s, ref in ((1.0, c), (0.0, u), (2.5, u + 2.5 * (c - u)), (-0.5, u - 0.5 * (c - u))):
        got = draw(lg, 0.7, False, None, None, rule, s).view(-1)
        want = rule(torch.cat([ref, ref]) / 0.7)[:b].argmax(dim=-1)
        assert torch.equal(got[:b], want) and torch.equal(got[b:], want), s
    torch.manual_seed(0)
    got = draw(lg, 1.0, True, 10, 0.9, rule, 3.0).view(-1)
    assert torch.equal(got[:b], got[b:]) and bool((got != 0).all())
    # cfg=None keeps the plain draw on all 2B rows
    assert torch.equal(draw(lg, 0.7, False, None, None, rule).view(-1), rule(lg[:, -1] / 0.7).argmax(dim=-1))
