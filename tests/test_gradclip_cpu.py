"""Gradient clipping, the parts that need no GPU: train.py's flags, and the reference formula that tests/test_gpu_gradclip.py holds
the kernels to, checked against torch.nn.utils.clip_grad_norm_ itself."""
import numpy as np
import torch

import train


def test_parser_takes_the_flags_and_defaults_are_off():
    opt, unknown = train.get_parser().parse_known_args(["-b", "x.yml"])
    assert opt.gradient_clip_val == 0.0 and opt.skip_nonfinite_grads is False and unknown == []
    opt, unknown = train.get_parser().parse_known_args(["-b", "x.yml", "--gradient_clip_val", "1.5", "--skip_nonfinite_grads"])
    assert opt.gradient_clip_val == 1.5 and opt.skip_nonfinite_grads is True and unknown == []


def test_flags_left_the_ignored_list():
    argv = ["-b", "x.yml", "--gradient_clip_val", "0.5", "--skip_nonfinite_grads", "--accumulate_grad_batches", "2",
            "model.params.lossconfig.params.disc_factor=0", "--fast_dev_run"]
    _, unknown = train.get_parser().parse_known_args(argv)
    dot, ignored = train.split_unknown(unknown)
    assert dot == ["model.params.lossconfig.params.disc_factor=0"]
    assert ignored == ["--accumulate_grad_batches", "2", "--fast_dev_run"]      # other Trainer flags: still reported, as before


def _reference_clip(grads, clip):
    """what the GPU test uses: the fp64 norm of all gradients, coef32 = float32(min(1, clip / (norm64 + 1e-6))), products in fp32"""
    norm64 = float(np.linalg.norm(np.concatenate([g.ravel().astype(np.float64) for g in grads])))
    coef32 = np.float32(min(1.0, clip / (norm64 + 1e-6)))
    return norm64, coef32, [g * coef32 for g in grads]


def test_reference_formula_is_torch_clip_grad_norm():
    """torch computes norm and coefficient in fp32, the reference in fp64 rounded once: the norms agree to 1e-6 relative, the
    coefficients to one fp32 ulp, so each scaled gradient to |g| * ulp(coef) plus the rounding of the two products (half an ulp each)"""
    rs = np.random.RandomState(5)
    shapes = [(5,), (3, 4), (7,), (1,)]
    for case, clip in enumerate((0.05, 1.0, 3.0, 1e3)):
        grads = [rs.standard_normal(s).astype(np.float32) * np.float32(10.0 ** rs.randint(-3, 2)) for s in shapes]
        params = [torch.nn.Parameter(torch.zeros(s)) for s in shapes]
        for p, g in zip(params, grads):
            p.grad = torch.from_numpy(g.copy())
        tnorm = float(torch.nn.utils.clip_grad_norm_(params, clip))
        norm64, coef32, scaled = _reference_clip(grads, clip)
        assert abs(tnorm - norm64) <= 1e-6 * norm64, case
        for p, g, s in zip(params, grads, scaled):
            got = p.grad.numpy()
            slack = np.abs(g) * np.spacing(coef32) + np.spacing(np.abs(s))
            assert np.all(np.abs(got - s) <= slack), (case, clip, float(coef32))
        if norm64 + 1e-6 <= clip:
            assert coef32 == 1.0 and all(np.array_equal(p.grad.numpy(), g) for p, g in zip(params, grads))
    # both regimes were exercised
    assert _reference_clip(grads, 1e3)[1] == 1.0 and _reference_clip(grads, 1e-3)[1] < 0.5
