"""Host-side mirror of reference/modules/vector_quantization/quantize_codebook_mask.py (MaskVectorQuantize: the gradient-trained
codebook) on the kernels of csrc/vq_trained.hip and the existing VQ kernels.

Same constructor kwargs and defaults, the same state dict (`initted` [1], `cluster_size` [1,K], `embedding.weight` [K,D] without a
padding row) and the same return signatures.  What differs from the EMA quantiser (quantize.py):
  * the codebook is an nn.Embedding trained by the optimizer through the codebook term of the loss: `bwd` accumulates its gradient
    (a masked, weighted scatter-reduction: dvq_vq_codebook_grad) into `embedding.weight.grad`;
  * the search is L2 or cosine, and at a sampling temperature > 0 it adds Gumbel noise to every score (dvq_vq_sample_argmax: no
    [N,K] matrix; the noise is a counter-based hash whose {seed, counter} state lives in device memory and advances on the stream,
    so a recorded training step draws fresh noise on every replay).  The reference's torch RNG stream cannot be reproduced;
  * the loss is normalised by the mask ratio N / sum(mask), computed on the device (no host read in fwd / bwd);
  * the optional orthogonality regulariser w * sum((W W^T - I)^2) / K^2, W = normalize(E), costs two K x K x D products per step;
  * the optional k-means initialisation runs eagerly on the first training forward (vq_argmin + vq_ema_stats per round).
Differences to the reference that matter: temp == 0 with L2 scores takes the mathematically exact argmin (lowest index on ties), where
the reference takes the fp32 argmax of its expanded formula; k-means under data parallelism raises (see _kmeans_init).
"""
from __future__ import annotations

import torch
import torch.distributed as dist
import torch.nn as nn

from . import kernels as K
from . import runtime as rt
from .layers import Tape, _grad_buf, to_nchw, to_nhwc


class MaskVectorQuantize(nn.Module):
    """quantize_codebook_mask.py:15-165."""

    takes_temperature = True        # fwd() accepts `temp`: DualGrainVQModel.ae_fwd passes its quant_sample_temperature (the one source)

    def __init__(self, codebook_size, codebook_dim=None, kmeans_init=False, kmeans_iters=10, use_cosine_sim=False,
                 channel_last=False, accept_image_fmap=True, commitment_beta=0.25, orthogonal_reg_weight=0.,
                 activate_mask_quantize=True):
        super().__init__()
        self.codebook_size = codebook_size
        self.codebook_dim = codebook_dim
        self.accept_image_fmap = accept_image_fmap
        self.channel_last = channel_last
        self.use_cosine_sim = use_cosine_sim
        self.beta = commitment_beta
        self.embedding = nn.Embedding(codebook_size, codebook_dim)
        if not kmeans_init:
            self.embedding.weight.data.uniform_(-1.0 / codebook_size, 1.0 / codebook_size)
        else:
            self.embedding.weight.data.zero_()
        self.kmeans_iters = kmeans_iters
        self.register_buffer("initted", torch.Tensor([not kmeans_init]))
        self.register_buffer("cluster_size", torch.zeros(1, codebook_size))
        self.orthogonal_reg_weight = orthogonal_reg_weight
        self.activate_mask_quantize = activate_mask_quantize
        if not accept_image_fmap:
            raise NotImplementedError("only accept_image_fmap=True is on the shipped configs' path")
        self.sample_temperature = 0.0   # what fwd() uses when a caller passes no temperature (the model always passes its own)
        self.kmeans_perm = None         # optional injected starting rows of the k-means initialisation (tests)
        self._initted_host = None       # host copy of `initted` (None = unknown: read the buffer once)
        self._prep = None               # (key, prepared planes) of the eval-mode search

    # -- state ----------------------------------------------------------------------------------------
    def _load_from_state_dict(self, *a, **k):
        super()._load_from_state_dict(*a, **k)
        self._initted_host, self._prep = None, None

    def is_initted(self) -> bool:
        """`initted` != 0.  Reads the buffer (a host sync) only until the answer is yes: k-means runs once, then never again"""
        if self._initted_host is not True:
            self._initted_host = bool(self.initted.detach().reshape(-1)[0].item() != 0)
        return self._initted_host

    def _rng(self, device):
        """device-resident {seed, counter} of the Gumbel noise and of the k-means row sampler (seeded from torch's seed; the counter
        advances on the stream: no host state, replays inside a recorded training step draw fresh noise)"""
        st = getattr(self, "_rng_state", None)
        if st is None or st.device != device:
            # the hash input is the LOCAL row number: ranks seeded alike would draw the same noise for their n-th rows, so the rank is
            # mixed into the seed.  The k-means row sampler shares this state; it runs once, before any noisy search.
            rank = dist.get_rank() if dist.is_available() and dist.is_initialized() else 0
            seed = (torch.initial_seed() + 0x9E3779B97F4A7C15 * rank) & 0x7FFFFFFFFFFFFFFF
            st = torch.tensor([seed, 0], dtype=torch.int64).to(device)
            self._rng_state = st
        return st

    def _weight(self):
        return self.embedding.weight.detach()

    def invalidate(self):
        """drop the eval-mode search's prepared planes.  Their key follows the runtime's parameter epochs, the weight's storage and its
        version counter; a write through `embedding.weight.data` moves none of these -- call this after one (load_state_dict does)"""
        self._prep = None

    # -- k-means initialisation (common_utils.py:116-156) ---------------------------------------------
    @torch.no_grad()
    def _kmeans_init(self, flat):
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            raise NotImplementedError(
                "kmeans_init under data parallelism: the reference runs k-means on every rank's own batch with its own sampled rows "
                "(all_reduce_fn is a no-op there), which leaves every rank with a DIFFERENT codebook; initialise on one process and "
                "load the checkpoint instead")
        k, d = self.codebook_size, self.codebook_dim
        x = K.cast(flat.reshape(-1, d), torch.float32).contiguous()
        n = x.shape[0]
        if self.kmeans_perm is not None:
            rows = self.kmeans_perm.to(x.device).reshape(-1)[:k].contiguous()
        elif n >= k:
            rows = K.sample_rows(k, n, self._rng(x.device))                  # = randperm(n)[:k]
        else:
            rows = torch.randint(0, n, (k,), device=x.device)                  # common_utils.py:47-48
        means = K.vq_embed(x, rows)
        bins = torch.zeros(k, dtype=torch.float32, device=x.device)
        for _ in range(self.kmeans_iters):
            buckets = K.vq_argmin(x, means, impl=rt.impl())                    # nearest mean by L2, exact, lowest index on ties
            stats = K.vq_ema_stats(x, buckets, k)                              # [K, D+1] = (sums | count)
            bins = stats[:, d]
            empty = (bins == 0).unsqueeze(1)
            means = torch.where(empty, means, stats[:, :d] / bins.clamp(min=1.0).unsqueeze(1)).contiguous()
        self.embedding.weight.data.copy_(means)
        self.cluster_size.copy_(bins.view(1, k))
        self.initted.fill_(1.0)
        self._initted_host, self._prep = True, None

    # -- search -----------------------------------------------------------------------------------------
    def _search(self, flat, w, temp):
        k, d = w.shape
        # the optimizer rewrites the weight between training forwards -- inside a recorded step without running any Python -- so a
        # training forward prepares anew, as part of the step; only eval-mode searches keep their prepared planes
        fresh = self.training or rt.capturing()
        exact = temp == 0 and not self.use_cosine_sim
        key = (exact, self.use_cosine_sim, rt.param_epoch(self.embedding.weight), rt.codebook_epoch(), w.data_ptr(), w._version)
        prep = None if fresh or self._prep is None or self._prep[0] != key else self._prep[1]
        if exact:
            # the EMA quantiser's exact search (quantize.VQEmbedding.find_nearest_embedding)
            if prep is None and d in (64, 128, 256):
                prep = K.vq_prepare(w)
                self._prep = None if fresh else (key, prep)
            return K.vq_argmin(flat, w, prep, impl=rt.impl())
        if prep is None:
            prep = K.vq_trained_prepare(w, self.use_cosine_sim)
            self._prep = None if fresh else (key, prep)
        return K.vq_sample_argmax(flat, prep, k, self.use_cosine_sim, temp, self._rng(flat.device) if temp > 0 else None, codebook=w)

    # -- NHWC core used by the model -------------------------------------------------------------------
    def fwd(self, h, mask, tape, temp=None):
        """h NHWC [B,H,W,D] (compute dtype), mask fp32 [B,H,W] or None -> (x_q NHWC, loss fp32 scalar tensor, idx int64 [B,H,W])"""
        b, hh, ww, d = h.shape
        flat = h.view(-1, d)
        if self.training and not self.is_initted():
            self._kmeans_init(flat)
        temp = float(self.sample_temperature if temp is None else temp)
        mflat = None
        if mask is not None and self.activate_mask_quantize:
            mflat = mask.reshape(-1)
            if mflat.dtype != torch.float32 or not mflat.is_contiguous():
                mflat = mflat.float().contiguous()
        w = self._weight()
        idx = self._search(flat, w, temp)
        xq, loss_sum = K.vq_gather_loss(flat, w, idx, mflat)      # x + (e - x): the straight-through value; sum of m |e - x|^2
        n_el = flat.numel()
        ratio = None if mflat is None else K.vq_mask_ratio(mflat)  # 1 / mean(mask), on the device
        loss = (loss_sum * ((1.0 + self.beta) / n_el)).to(torch.float32)
        if ratio is not None:
            loss = loss * ratio
        ortho = None
        if self.orthogonal_reg_weight > 0.:
            # eq. (2) of arXiv 2112.00384: W = normalize(E), w * sum((W W^T - I)^2) / K^2.  fp32 operands whatever the compute dtype
            k = w.shape[0]
            wn, inv = K.vq_rownorm(w)
            g = K.gemm_nt(wn.view(-1), wn.view(-1), k, k, d, d, d, k)
            loss = loss + K.vq_ortho_sumsq(g, k, self.orthogonal_reg_weight / float(k * k))       # g is now W W^T - I
            ortho = (wn, inv, g)
        if tape is not None:
            tape.s.update(h=flat, idx=idx, mask=mflat, n_el=n_el, ratio=ratio, ortho=ortho)
        return xq.view(b, hh, ww, d), loss.reshape(()), idx.view(b, hh, ww)

    def bwd(self, g_xq, g_loss, tape):
        """g_xq NHWC grad of x_q, g_loss device scalar (grad of the loss) -> grad of h (NHWC); the codebook's gradient is accumulated
        into embedding.weight.grad.  The weight is the forward's: nothing rewrites it between a forward and its backward."""
        s = tape.s
        d = s["h"].shape[1]
        w = self._weight()
        base = g_loss.to(torch.float32).reshape(1) * (2.0 / s["n_el"])
        if s["ratio"] is not None:
            base = base * s["ratio"]
        dx = K.vq_backward(g_xq.reshape(-1, d), s["h"], w, s["idx"], s["mask"], (base * self.beta).contiguous())
        if self.embedding.weight.requires_grad:
            grad = _grad_buf(self.embedding.weight)
            K.vq_codebook_grad(s["h"], w, s["idx"], s["mask"], base.contiguous(), grad)
            if s["ortho"] is not None:
                wn, inv, g = s["ortho"]
                k = w.shape[0]
                dw = K.gemm_tn(g, wn.view(-1), k, k, d, k, d, d)               # G^T W = G W (G is symmetric); d sum(G^2) / dW = 4 G W
                K.vq_rownorm_bwd(wn, inv, dw.view(k, d), g_loss.to(torch.float32).reshape(1).contiguous(),
                                 4.0 * self.orthogonal_reg_weight / float(k * k), grad)
        return dx.view(g_xq.shape)

    # -- reference signature ---------------------------------------------------------------------------
    def forward(self, x, temp=0., codebook_mask=None):
        """x [B,D,H,W] -> (x_q [B,D,H,W], loss, (None, None, idx [B,H,W]))  (quantize_codebook_mask.py:77-144)"""
        mask = None
        if codebook_mask is not None and self.activate_mask_quantize:
            mask = codebook_mask.reshape(codebook_mask.shape[0], *codebook_mask.shape[-2:]).to(torch.float32).contiguous()
        xq, loss, idx = _MaskVQFn.apply(self, x, mask, float(temp), self.embedding.weight)
        return xq, loss, (None, None, idx)

    @torch.no_grad()
    def get_codebook_entry(self, indices, shape=None, *kwargs):
        z_q = K.vq_embed(self._weight(), indices.contiguous(), torch.float32)     # (batch, height, width, channel)
        if shape is not None:
            z_q = z_q.view(shape).permute(0, 3, 1, 2).contiguous()
        return z_q

    @torch.no_grad()
    def embed_code_with_depth(self, code, to_latent_shape=False):
        """code [..., depth] -> (embeds [..., depth, D], None)  (quantize_codebook_mask.py:155-165)"""
        if to_latent_shape:
            raise NotImplementedError("to_latent_shape: the reference calls a method this class does not define")
        return K.vq_embed(self._weight(), code.contiguous(), torch.float32), None


class _MaskVQFn(torch.autograd.Function):
    """fwd / bwd as one autograd node; `weight` is an input only so that the node exists when the codebook alone needs a gradient
    (its gradient is accumulated into weight.grad by bwd, like every parameter gradient of the package)"""

    @staticmethod
    def forward(ctx, module, x, mask, temp, weight):
        ctx.module, ctx.in_dtype = module, x.dtype
        ctx.tape = Tape()
        with torch.no_grad():
            h = to_nhwc(x, rt.compute_dtype())
            xq, loss, idx = module.fwd(h, mask, ctx.tape, temp)
            ctx.out_shape = tuple(xq.shape)
            xq = to_nchw(K.cast(xq, x.dtype))
        ctx.mark_non_differentiable(idx)
        return xq, loss, idx

    @staticmethod
    def backward(ctx, g_xq, g_loss, _g_idx):
        with torch.no_grad():
            h = ctx.tape.s["h"]
            if g_loss is None:
                g_loss = torch.zeros((), device=h.device)
            if g_xq is None:            # only the loss was used
                g_nhwc = torch.zeros(ctx.out_shape, dtype=h.dtype, device=h.device)
            else:
                g_nhwc = to_nhwc(g_xq, rt.compute_dtype())
            dx = ctx.module.bwd(g_nhwc, g_loss, ctx.tape)
            dx = to_nchw(K.cast(dx, ctx.in_dtype))
        return None, dx, None, None, None
