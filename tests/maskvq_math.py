"""The gradient-trained codebook (MaskVectorQuantize) restated in torch-CPU arithmetic, and the deterministic inputs of its fixtures.

Shared by tools/gen_golden_maskvq.py (which feeds the inputs to the REFERENCE class and stores its outputs in tests/golden/maskvq.npz),
tests/test_maskvq_cpu.py (this restatement reproduces the fixture) and tests/test_gpu_maskvq.py (the kernels against both).

Formulas (N = B H W rows x_n of dimension D, codebook E [K,D], m = mask broadcast over D or 1):
  scores   L2: s[n,k] = -|x_n|^2 - |e_k|^2 + 2 x_n.e_k        cosine: s[n,k] = x^_n . e^_k  (v^ = v / max(|v|, 1e-12))
  pick     argmax_k s (temp 0) or argmax_k (s / temp + g), lowest index on ties
  output   x_q = E[idx] (raw rows), straight-through
  loss     ratio (1 + beta) mean(m (x_q - x)^2), ratio = 1 / mean(m)      [+ w sum((W W^T - I)^2) / K^2, W = normalize(E)]
  grads    dx_n = g_xq,n + g_loss ratio 2 beta / (N D) m_n (x_n - e_idx),  dE_k = g_loss ratio 2 / (N D) sum_{idx_n = k} m_n (e_k - x_n)
"""
import numpy as np
import torch
import torch.nn.functional as F

BETA = 0.25

# ---- fixture inputs -----------------------------------------------------------------------------------------------------------------
# temp-0 search: (B, D, H, W, K); the last two are the N = 1 and the K = 8 edge
SEARCH_SHAPES = [(2, 64, 8, 8, 512), (3, 256, 8, 8, 1024), (2, 72, 4, 6, 100), (1, 64, 1, 1, 512), (2, 128, 4, 4, 8)]
# module forward / backward: name -> (cosine, pass a mask, activate_mask_quantize)
MODULE_VARIANTS = {"l2_mask": (False, True, True), "cos_mask": (True, True, True), "l2_nomask": (False, False, True),
                   "l2_inactive": (False, True, False)}
MODULE_SHAPE = (2, 64, 6, 8, 128)            # (B, D, H, W, K)
ORTHO_SHAPE = (2, 64, 4, 4, 128)             # K 128, D 64
ORTHO_W = 10.0
KMEANS_SHAPE = (2, 64, 16, 16, 16)           # N 512, K 16, D 64
KMEANS_ITERS = 10
G_LOSS = 3.0                                 # the scalar the fixtures' objective multiplies the loss with


def rng(tag, seed=0):
    h = 0
    for ch in tag:
        h = (h * 131 + ord(ch)) % (2 ** 31 - 1)
    return np.random.RandomState((h + 7919 * seed) % (2 ** 32))


def search_inputs(shape, seed=0):
    """x [B,D,H,W], E [K,D] fp32, standard normal"""
    b, d, h, w, k = shape
    r = rng("search" + ",".join(map(str, shape)), seed)
    return r.standard_normal((b, d, h, w)).astype(np.float32), r.standard_normal((k, d)).astype(np.float32)


def module_inputs(tag, shape, seed=0):
    """x [B,D,H,W], E [K,D], mask [B,1,H,W] in {0.25, 1} (the dual-grain mask's two values), upstream gradient of x_q [B,D,H,W]"""
    b, d, h, w, k = shape
    r = rng("module" + tag, seed)
    x = r.standard_normal((b, d, h, w)).astype(np.float32)
    e = (0.7 * r.standard_normal((k, d))).astype(np.float32)
    mask = np.where(r.uniform(size=(b, 1, h, w)) < 0.5, 0.25, 1.0).astype(np.float32)
    g = r.standard_normal((b, d, h, w)).astype(np.float32) / np.float32(b * d * h * w)
    return x, e, mask, g


def kmeans_inputs(seed=0):
    """clustered rows (K centres + noise) as x [B,D,H,W], and K distinct starting row indices"""
    b, d, h, w, k = KMEANS_SHAPE
    r = rng("kmeans", seed)
    n = b * h * w
    centres = r.standard_normal((k, d)).astype(np.float32)
    rows = centres[r.randint(0, k, size=n)] + (0.5 * r.standard_normal((n, d))).astype(np.float32)
    x = np.ascontiguousarray(rows.reshape(b, h, w, d).transpose(0, 3, 1, 2)).astype(np.float32)
    perm = r.permutation(n)[:k].astype(np.int64)
    return x, perm


def rows_of(x):
    """[B,D,H,W] -> [B H W, D] in the quantiser's row order"""
    x = torch.as_tensor(x)
    return x.permute(0, 2, 3, 1).reshape(-1, x.shape[1])


def bf16_round(a):
    return torch.as_tensor(a).to(torch.bfloat16).to(torch.float32).numpy()


# ---- the formulas -------------------------------------------------------------------------------------------------------------------
def scores(rows, e, cosine, dtype=torch.float64):
    """[N,K] scores in `dtype` arithmetic"""
    x, e = torch.as_tensor(rows).to(dtype), torch.as_tensor(e).to(dtype)
    if cosine:
        return F.normalize(x, p=2, dim=-1, eps=1e-12) @ F.normalize(e, p=2, dim=-1, eps=1e-12).t()
    return -(x ** 2).sum(1, keepdim=True) - (e ** 2).sum(1) + 2.0 * (x @ e.t())


def pick(s, temp=0.0, noise=None):
    """argmax_k (s / temp + noise) (temp 0: of s), lowest index on ties -> (idx int64 [N], top-2 gap of the maximised values [N])"""
    v = s if temp == 0 else s / temp + torch.as_tensor(noise).to(s.dtype)
    vmax = v.max(dim=1, keepdim=True).values
    idx = torch.argmax((v == vmax).to(torch.int8), dim=1)          # first position of the maximum
    if v.shape[1] > 1:
        top2 = torch.topk(v, 2, dim=1).values
        gap = top2[:, 0] - top2[:, 1]
    else:
        gap = torch.full((v.shape[0],), float("inf"), dtype=v.dtype)
    return idx, gap


def ortho_term(e, w):
    """w sum((W W^T - I)^2) / K^2, W = normalize(E); differentiable"""
    wn = F.normalize(e, p=2, dim=-1, eps=1e-12)
    k = e.shape[0]
    g = wn @ wn.t() - torch.eye(k, dtype=e.dtype)
    return w * (g ** 2).sum() / (k * k)


def forward_backward(x, e, mask, g_xq, cosine=False, activate_mask=True, ortho_w=0.0, beta=BETA, g_loss=G_LOSS, temp=0.0, noise=None,
                     dtype=torch.float64):
    """the module's forward and the gradients of  sum(x_q * g_xq) + g_loss * loss  w.r.t. x and E, by autograd over the formulas above.
    x, g_xq [B,D,H,W]; mask [B,1,H,W] or None -> dict(x_q [B,D,H,W], loss, idx [B,H,W], dx [B,D,H,W], dE [K,D], ortho)"""
    xt = torch.as_tensor(x).to(dtype).clone().requires_grad_(True)
    et = torch.as_tensor(e).to(dtype).clone().requires_grad_(True)
    b, d, h, w = xt.shape
    rows = xt.permute(0, 2, 3, 1).reshape(-1, d)
    with torch.no_grad():
        idx, _ = pick(scores(rows, et, cosine, dtype), temp, noise)
    xq = et[idx]
    if mask is not None and activate_mask:
        m = torch.as_tensor(mask).to(dtype).permute(0, 2, 3, 1).reshape(-1, 1)
        ratio = 1.0 / m.mean()
        loss = ratio * beta * ((xq.detach() - rows) ** 2 * m).mean() + ratio * ((xq - rows.detach()) ** 2 * m).mean()
    else:
        loss = beta * ((xq.detach() - rows) ** 2).mean() + ((xq - rows.detach()) ** 2).mean()
    ortho = ortho_term(et, ortho_w) if ortho_w > 0 else None
    if ortho is not None:
        loss = loss + ortho
    xq_st = rows + (xq - rows).detach()
    xq_img = xq_st.reshape(b, h, w, d).permute(0, 3, 1, 2)
    obj = (xq_img * torch.as_tensor(g_xq).to(dtype)).sum() + g_loss * loss
    obj.backward()
    return dict(x_q=xq_img.detach().numpy(), loss=float(loss.detach()), idx=idx.reshape(b, h, w).numpy(), dx=xt.grad.numpy(), dE=et.grad.numpy(),
                ortho=None if ortho is None else float(ortho.detach()))


def kmeans(rows, perm, k, iters, dtype=torch.float64):
    """k-means as the reference runs it (common_utils.py:116-156) from the starting rows `perm`: nearest mean by L2, per-cluster means,
    empty clusters keep their mean -> (means [K,D], bins [K] of the last round, assignments of every round [iters, N])"""
    x = torch.as_tensor(rows).to(dtype)
    means = x[torch.as_tensor(perm)[:k]].clone()
    hist = []
    bins = torch.zeros(k, dtype=dtype)
    for _ in range(iters):
        d2 = (x ** 2).sum(1, keepdim=True) + (means ** 2).sum(1) - 2.0 * (x @ means.t())
        dmin = d2.min(dim=1, keepdim=True).values
        buckets = torch.argmax((d2 == dmin).to(torch.int8), dim=1)
        hist.append(buckets.numpy())
        bins = torch.bincount(buckets, minlength=k).to(dtype)
        sums = torch.zeros(k, x.shape[1], dtype=dtype).index_add_(0, buckets, x)
        new = sums / bins.clamp(min=1.0).unsqueeze(1)
        means = torch.where((bins == 0).unsqueeze(1), means, new)
    return means.numpy(), bins.numpy(), np.stack(hist)


def rel_to_max(got, ref):
    """max |got - ref| / max |ref|: the project's parity measure"""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float(np.abs(got - ref).max()) / max(1e-30, float(np.abs(ref).max()))
