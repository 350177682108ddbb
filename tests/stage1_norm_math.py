"""torch fp64 restatement of the stage-1 normalisation layers (csrc/groupnorm.hip; docs/design/26-groupnorm-kernel-pins.md): GroupNorm
with a fused activation and its backward, the per-(n, c) {scale, shift} table of the fused conv prologue, BatchNorm2d in training and
eval mode, ActNorm.  What the kernels must compute, written from the definitions without reference to how they compute it, in plain
tensor operations so that the same functions run on the CPU and on a device.  Nothing of the package is imported.

Layout: x [N, ..., C], channels last; a group is `C / groups` adjacent channels; statistics per (n, group) over every pixel."""
import torch

ACT_NONE, ACT_SWISH, ACT_LRELU = 0, 1, 2
LRELU_SLOPE = 0.2


def f64(a, device=None):
    t = a if torch.is_tensor(a) else torch.as_tensor(a)
    return t.to(device=device if device is not None else t.device, dtype=torch.float64)


def bf16_round(a):
    """fp32 tensor -> the nearest bf16 value (ties to even), as fp32"""
    return torch.as_tensor(a, dtype=torch.float32).to(torch.bfloat16).float()


def _grouped(x, groups):
    """[N, ..., C] -> [N, P, G, C / G]"""
    n, c = x.shape[0], x.shape[-1]
    assert c % groups == 0
    return x.reshape(n, -1, groups, c // groups)


def _per_channel(v, c):
    """[N, G] -> [N, 1, C]: every channel gets the value of its group"""
    return v.repeat_interleave(c // v.shape[1], dim=1)[:, None, :]


def group_sums(x, groups):
    """-> (sum x, sum x^2, sum |x|), each [N, G]: what the statistics kernel accumulates, and the magnitude of its terms"""
    v = _grouped(f64(x), groups)
    return v.sum(dim=(1, 3)), (v * v).sum(dim=(1, 3)), v.abs().sum(dim=(1, 3))


def group_mean_var(x, groups):
    """two-pass mean and biased variance per (n, group), each [N, G]"""
    v = _grouped(f64(x), groups)
    mean = v.mean(dim=(1, 3))
    var = ((v - mean[:, None, :, None]) ** 2).mean(dim=(1, 3))
    return mean, var


def rstd_of(var, eps):
    return 1.0 / torch.sqrt(var + float(eps))


def scale_shift(mean, rstd, gamma, beta):
    """{scale, shift} = {rstd gamma, beta - mean scale} -> [N, C, 2]"""
    gamma, beta = f64(gamma), f64(beta)
    c = gamma.numel()
    scale = _per_channel(rstd, c)[:, 0] * gamma
    shift = beta - _per_channel(mean, c)[:, 0] * scale
    return torch.stack([scale, shift], dim=-1)


def act(z, kind):
    if kind == ACT_SWISH:
        return z * torch.sigmoid(z)
    if kind == ACT_LRELU:
        return torch.where(z > 0, z, LRELU_SLOPE * z)
    assert kind == ACT_NONE
    return z


def act_grad(z, kind):
    if kind == ACT_SWISH:
        s = torch.sigmoid(z)
        return s * (1.0 + z * (1.0 - s))
    if kind == ACT_LRELU:
        return torch.where(z > 0, torch.ones_like(z), torch.full_like(z, LRELU_SLOPE))
    assert kind == ACT_NONE
    return torch.ones_like(z)


def normalized(x, mean, rstd):
    """xhat = (x - mean) rstd as [N, P, C]"""
    x = f64(x)
    c = x.shape[-1]
    return (x.reshape(x.shape[0], -1, c) - _per_channel(mean, c)) * _per_channel(rstd, c)


def gn_forward(x, gamma, beta, groups, eps, kind=ACT_NONE, mean=None, rstd=None):
    """y = act(xhat gamma + beta) -> (y, z, mean, rstd); mean / rstd [N, G]: given statistics instead of those of x"""
    x = f64(x)
    if mean is None:
        mean, var = group_mean_var(x, groups)
        rstd = rstd_of(var, eps)
    z = normalized(x, mean, rstd) * f64(gamma) + f64(beta)
    return act(z, kind).reshape(x.shape), z.reshape(x.shape), mean, rstd


def gn_backward(x, dy, gamma, beta, groups, kind, mean, rstd, addend=None, fixed_stats=False):
    """mean / rstd [N, G]: the statistics the forward saved.  -> (dx, dgamma, dbeta)
         dz = dy act'(z),  dbeta = sum dz,  dgamma = sum dz xhat,
         dx = rstd (dz gamma - mean_g(dz gamma) - xhat mean_g(dz gamma xhat)) + addend,
       fixed_stats (the statistics are constants, not functions of x): dx = rstd gamma dz + addend"""
    x, dy, gamma, beta = f64(x), f64(dy), f64(gamma), f64(beta)
    n, c = x.shape[0], x.shape[-1]
    xh = normalized(x, mean, rstd)
    dz = dy.reshape(n, -1, c) * act_grad(xh * gamma + beta, kind)
    dbeta, dgamma = dz.sum(dim=(0, 1)), (dz * xh).sum(dim=(0, 1))
    g = dz * gamma
    r = _per_channel(rstd, c)
    if fixed_stats:
        dx = r * g
    else:
        m1 = _per_channel(_grouped(g, groups).mean(dim=(1, 3)), c)
        m2 = _per_channel(_grouped(g * xh, groups).mean(dim=(1, 3)), c)
        dx = r * (g - m1 - xh * m2)
    dx = dx.reshape(x.shape)
    if addend is not None:
        dx = dx + f64(addend)
    return dx, dgamma, dbeta


# ---- BatchNorm2d: GroupNorm with one group per channel over the whole batch --------------------------------------------------------------
def bn_batch_stats(x):
    """x [N, ..., C] -> per-channel mean and biased variance over every other axis"""
    mean, var = group_mean_var(f64(x).reshape(1, -1, x.shape[-1]), x.shape[-1])
    return mean[0], var[0]


def bn_running_update(x, running_mean, running_var, momentum):
    """-> the buffers after one training forward: (1 - momentum) old + momentum new, the new variance unbiased"""
    mean, var = bn_batch_stats(x)
    cnt = x.numel() // x.shape[-1]
    unbiased = var * (cnt / max(cnt - 1.0, 1.0))
    return (1.0 - momentum) * f64(running_mean) + momentum * mean, (1.0 - momentum) * f64(running_var) + momentum * unbiased


def bn_train(x, gamma, beta, eps, kind=ACT_NONE):
    y, _, _, _ = gn_forward(f64(x).reshape(1, -1, x.shape[-1]), gamma, beta, x.shape[-1], eps, kind)
    return y.reshape(x.shape)


def bn_eval(x, running_mean, running_var, gamma, beta, eps, kind=ACT_NONE):
    z = (f64(x) - f64(running_mean)) / torch.sqrt(f64(running_var) + float(eps)) * f64(gamma) + f64(beta)
    return act(z, kind)


# ---- ActNorm -----------------------------------------------------------------------------------------------------------------------------
def actnorm_forward(x, loc, scale, kind=ACT_NONE):
    """h = scale (x + loc) per channel"""
    return act(f64(scale).reshape(-1) * (f64(x) + f64(loc).reshape(-1)), kind)
