"""gather_features + ClipLoss with the reference's signatures (reference loss.py:48-182).

The arithmetic — the tall-skinny `logit_scale * A @ B.T` GEMM, both softmax cross-entropies and
their backward — runs in hand-written HIP kernels (fp32: this is the path the 1e-3 logits/loss
parity bar applies to).  The logits matrix is formed once, turned into d(logits) in place, and
consumed by two GEMMs; the label vector is never materialised (labels are `arange + offset`).
Collectives are torch.distributed (RCCL on MI355X, gloo in CPU tests).
"""
from typing import Optional

import torch
import torch.nn as nn

try:
    import torch.distributed.nn  # noqa: F401
    from torch import distributed as dist

    has_distributed = True
except ImportError:  # pragma: no cover
    has_distributed = False

from . import ops
from .trace import phase


# --------------------------------------------------------------------------- collectives
def _reduce_scatter_available() -> bool:
    """RCCL has reduce-scatter; gloo (CPU tests, and the two-ranks-on-one-GPU test) does not.  Decided by the backend, not by
    the tensor's device.  A stand-in `dist` object (single-GPU simulations in the tests) without get_backend counts as having it."""
    get = getattr(dist, "get_backend", None)
    if get is None:
        return True
    try:
        return str(get()).lower() == "nccl"
    except (RuntimeError, ValueError):
        return True


class _AllGatherCat(torch.autograd.Function):
    """cat(all_gather(x)) with the reference's gather_with_grad semantics (loss.py:77-79):
    backward = reduce-scatter(SUM) of the gathered gradient (torch.distributed.nn.all_gather on
    NCCL).  One collective per tensor on a single contiguous [W*b, E] buffer."""

    @staticmethod
    def forward(ctx, x, rank, world_size):
        ctx.rank, ctx.world_size = rank, world_size
        x = x.contiguous()
        out = torch.empty((world_size * x.shape[0],) + tuple(x.shape[1:]), dtype=x.dtype, device=x.device)
        dist.all_gather_into_tensor(out, x)
        return out

    @staticmethod
    def backward(ctx, g):
        g = g.contiguous()
        b = g.shape[0] // ctx.world_size
        if _reduce_scatter_available():
            out = torch.empty((b,) + tuple(g.shape[1:]), dtype=g.dtype, device=g.device)
            dist.reduce_scatter_tensor(out, g, op=dist.ReduceOp.SUM)
        else:   # gloo has no reduce-scatter
            dist.all_reduce(g, op=dist.ReduceOp.SUM)
            out = g[ctx.rank * b:(ctx.rank + 1) * b].clone()
        return out, None, None


def _all_gather_nograd(x, world_size):
    x = x.contiguous()
    out = torch.empty((world_size * x.shape[0],) + tuple(x.shape[1:]), dtype=x.dtype, device=x.device)
    with torch.no_grad():
        dist.all_gather_into_tensor(out, x.detach())
    return out


def gather_features(
        image_features,
        text_features,
        local_loss=False,
        gather_with_grad=False,
        rank=0,
        world_size=1,
        use_horovod=False
):
    """reference loss.py:48-92 (torch.distributed branch).  Returns [N,E] x 2 in rank order."""
    assert has_distributed, 'torch.distributed did not import correctly, please use a PyTorch version with support.'
    if use_horovod:
        raise NotImplementedError("horovod is outside the MI355X hot path; use torch.distributed (RCCL)")
    if gather_with_grad:
        all_image_features = _AllGatherCat.apply(image_features, rank, world_size)
        all_text_features = _AllGatherCat.apply(text_features, rank, world_size)
    else:
        all_image_features = _all_gather_nograd(image_features, world_size)
        all_text_features = _all_gather_nograd(text_features, world_size)
        if not local_loss:
            # ensure grads for local rank when all_* features don't have a gradient (loss.py:85-88)
            b = image_features.shape[0]
            parts_i = [all_image_features[:rank * b], image_features, all_image_features[(rank + 1) * b:]]
            parts_t = [all_text_features[:rank * b], text_features, all_text_features[(rank + 1) * b:]]
            all_image_features = torch.cat(parts_i, dim=0)
            all_text_features = torch.cat(parts_t, dim=0)
    return all_image_features, all_text_features


# --------------------------------------------------------------------------- fused CE pieces
def _scaled_logits(a, b, scale):
    """(scale * a) @ b.T in fp32 on the HIP GEMM; returns (logits, scaled a)."""
    a_s = ops.scale_by_dev(a, scale)
    r, e = a.shape
    c = b.shape[0]
    z = torch.empty((r, c), dtype=torch.float32, device=a.device)
    ops.gemm_f32(r, c, e, a_s, e, 1, b, 1, e, z, c)
    return z, a_s


class _ContrastiveCE(torch.autograd.Function):
    """loss = w * sum_r CE(z[r,:], r + off)  [+ w * sum_c CE(z[:,c], c) when symmetric],
    z = (scale*a) @ b.T, w = 0.5 / rows.   Symmetric = the W==1 / global-loss case where
    logits_per_text is logits_per_image.T (loss.py:148-152).

    z is never written to memory (64 MiB at N = 4096, 1 GiB at N = 16384): the forward kernel keeps per-tile softmax
    statistics, the backward kernels recompute the logits tile by tile (csrc/loss_fused.hip).  Embed dims outside the
    fused kernels' list run the materialising kernels (_ContrastiveCEDense)."""

    @staticmethod
    def forward(ctx, a, b, scale, label_off: int, symmetric: bool):
        if a.shape[1] not in ops.FUSED_CE_DIMS:
            raise RuntimeError("internal: _ContrastiveCE called with an unsupported embed dim")
        with phase("loss.fwd"):
            a = a.contiguous().float()
            b = b.contiguous().float()
            scale = scale.detach().float().reshape(1).contiguous()
            r = a.shape[0]
            a_s = ops.scale_by_dev(a, scale)          # the reference scales the features, then multiplies (loss.py:145-152)
            w = 0.5 / r
            loss = torch.zeros((1,), dtype=torch.float32, device=a.device)
            if symmetric:
                assert r == b.shape[0] and label_off == 0
            lse_r, lse_c = ops.ce_fused_fwd(a_s, b, label_off, symmetric, w, w, loss)
        ctx.save_for_backward(a_s, b, scale, lse_r, lse_c if lse_c is not None else lse_r)
        ctx.label_off, ctx.symmetric, ctx.w = label_off, symmetric, w
        return loss.reshape(())

    @staticmethod
    def backward(ctx, gout):
        a_s, b, scale, lse_r, lse_c = ctx.saved_tensors
        off, w = ctx.label_off, ctx.w
        lse_c = lse_c if ctx.symmetric else None
        with phase("loss.bwd"):
            gout = gout.reshape(1).float().contiguous()
            need_a, need_b, need_s = ctx.needs_input_grad[0], ctx.needs_input_grad[1], ctx.needs_input_grad[2]
            da = db = ds = None
            dscale = torch.zeros((1,), dtype=torch.float32, device=a_s.device) if need_s else None
            if need_a or need_s:
                # rows of `a` own the walk: d(a) = scale * upstream * d(z) @ b; d(scale) = sum d(z)*z / scale rides along
                da = ops.ce_fused_bwd(a_s, b, lse_r, w, off, lse_c, w, 0, scale, gout, dscale, scale)
                if not need_a:
                    da = None
            if need_b:
                # rows of `b` own the walk: d(b) = upstream * d(z).T @ (scale*a)
                db = ops.ce_fused_bwd(b, a_s, lse_c, w, 0, lse_r, w, off, None, gout)
            if need_s:
                ds = (dscale * gout).reshape(())
        return da, db, ds, None, None


def contrastive_ce(a, b, scale, label_off: int, symmetric: bool):
    if a.shape[1] in ops.FUSED_CE_DIMS:
        return _ContrastiveCE.apply(a, b, scale, label_off, symmetric)
    return _ContrastiveCEDense.apply(a, b, scale, label_off, symmetric)


class _ContrastiveCEDense(torch.autograd.Function):
    """The same loss with the logits matrix in memory (embed dims the fused kernels are not instantiated for)."""

    @staticmethod
    def forward(ctx, a, b, scale, label_off: int, symmetric: bool):
        a = a.contiguous().float()
        b = b.contiguous().float()
        scale = scale.detach().float().reshape(1).contiguous()
        r, c = a.shape[0], b.shape[0]
        z, a_s = _scaled_logits(a, b, scale)
        w = 0.5 / r
        loss = torch.zeros((1,), dtype=torch.float32, device=a.device)
        lse_r = torch.empty((r,), dtype=torch.float32, device=a.device)
        ops.ce_rows(z, label_off, lse_r, w, loss)
        lse_c = None
        if symmetric:
            assert r == c and label_off == 0
            lse_c = torch.empty((c,), dtype=torch.float32, device=a.device)
            ops.ce_cols(z, lse_c, w, loss)
        ctx.save_for_backward(a_s, b, scale, z, lse_r, lse_c if lse_c is not None else lse_r)
        ctx.label_off, ctx.symmetric, ctx.w = label_off, symmetric, w
        return loss.reshape(())

    @staticmethod
    def backward(ctx, gout):
        a_s, b, scale, z, lse_r, lse_c = ctx.saved_tensors
        r, e = a_s.shape
        c = b.shape[0]
        dscale = torch.zeros((1,), dtype=torch.float32, device=z.device)
        # z -> dz in place (unit upstream gradient); consumes the saved logits
        ops.ce_grad(z, ctx.label_off, lse_r, ctx.w, lse_c if ctx.symmetric else None, ctx.w, scale, dscale)
        gout = gout.reshape(1).float()
        da = db = None
        if ctx.needs_input_grad[0]:
            t = torch.empty((r, e), dtype=torch.float32, device=z.device)
            ops.gemm_f32(r, e, c, z, c, 1, b, e, 1, t, e)                 # dz @ b
            da = ops.scale_by_dev(t, scale * gout, out=t)                  # * scale * upstream
        if ctx.needs_input_grad[1]:
            t = torch.empty((c, e), dtype=torch.float32, device=z.device)
            ops.gemm_f32(c, e, r, z, 1, c, a_s, e, 1, t, e)               # dz.T @ (scale*a)
            db = ops.scale_by_dev(t, gout, out=t)
        ds = (dscale * gout).reshape(()) if ctx.needs_input_grad[2] else None
        return da, db, ds, None, None


class _ScaledMatmul(torch.autograd.Function):
    """logits = (scale*a) @ b.T as a differentiable op (ClipLoss.get_logits API surface)."""

    @staticmethod
    def forward(ctx, a, b, scale):
        a = a.contiguous().float()
        b = b.contiguous().float()
        scale = scale.detach().float().reshape(1).contiguous()
        z, a_s = _scaled_logits(a, b, scale)
        ctx.save_for_backward(a, a_s, b, scale)
        return z

    @staticmethod
    def backward(ctx, dz):
        a, a_s, b, scale = ctx.saved_tensors
        dz = dz.contiguous().float()
        r, e = a.shape
        c = b.shape[0]
        t = torch.empty((r, e), dtype=torch.float32, device=dz.device)
        ops.gemm_f32(r, e, c, dz, c, 1, b, e, 1, t, e)
        da = ops.scale_by_dev(t, scale)
        db = torch.empty((c, e), dtype=torch.float32, device=dz.device)
        ops.gemm_f32(c, e, r, dz, 1, c, a_s, e, 1, db, e)
        ds = (t * a).sum().reshape(())
        return da, db, ds


class ClipLoss(nn.Module):
    """reference loss.py:95-182."""

    def __init__(
            self,
            local_loss=False,
            gather_with_grad=False,
            cache_labels=False,
            rank=0,
            world_size=1,
            use_horovod=False,
            **kwargs
    ):
        super().__init__()
        self.local_loss = local_loss
        self.gather_with_grad = gather_with_grad
        self.cache_labels = cache_labels
        self.rank = rank
        self.world_size = world_size
        self.use_horovod = use_horovod

        # cache state
        self.prev_num_logits = 0
        self.labels = {}

    def get_ground_truth(self, device, num_logits) -> torch.Tensor:
        # calculated ground-truth and cache if enabled
        if self.prev_num_logits != num_logits or device not in self.labels:
            labels = torch.arange(num_logits, device=device, dtype=torch.long)
            if self.world_size > 1 and self.local_loss:
                labels = labels + num_logits * self.rank
            if self.cache_labels:
                self.labels[device] = labels
                self.prev_num_logits = num_logits
        else:
            labels = self.labels[device]
        return labels

    def _gather(self, image_features, text_features):
        return gather_features(
            image_features, text_features,
            local_loss=self.local_loss, gather_with_grad=self.gather_with_grad,
            rank=self.rank, world_size=self.world_size, use_horovod=self.use_horovod)

    def get_logits(self, image_features, text_features, logit_scale, logit_bias=None):
        if self.world_size > 1:
            all_image_features, all_text_features = self._gather(image_features, text_features)
            if self.local_loss:
                logits_per_image = _ScaledMatmul.apply(image_features, all_text_features, logit_scale)
                logits_per_text = _ScaledMatmul.apply(text_features, all_image_features, logit_scale)
            else:
                logits_per_image = _ScaledMatmul.apply(all_image_features, all_text_features, logit_scale)
                logits_per_text = logits_per_image.T
        else:
            logits_per_image = _ScaledMatmul.apply(image_features, text_features, logit_scale)
            logits_per_text = _ScaledMatmul.apply(text_features, image_features, logit_scale)

        if logit_bias is not None:
            logits_per_image = logits_per_image + logit_bias
            logits_per_text = logits_per_text + logit_bias

        return logits_per_image, logits_per_text

    def forward(
            self,
            image_features=None,
            text_features=None,
            logit_scale=None,
            logit_bias=None,
            output_dict=False,
            logits_per_image=None,
            logits_per_text=None,
            **kwargs,
    ):
        # NB like the reference (loss.py:173) logit_bias is not applied here.
        if self.world_size > 1:
            all_image_features, all_text_features = self._gather(image_features, text_features)
            if self.local_loss:
                off = image_features.shape[0] * self.rank
                total_loss = (
                    contrastive_ce(image_features, all_text_features, logit_scale, off, False) +
                    contrastive_ce(text_features, all_image_features, logit_scale, off, False)
                )
            else:
                total_loss = contrastive_ce(all_image_features, all_text_features, logit_scale, 0, True)
        else:
            total_loss = contrastive_ce(image_features, text_features, logit_scale, 0, True)

        return {"total_loss": total_loss} if output_dict else total_loss


# --------------------------------------------------------------------------- ColClipLoss ("next" row)
class _MaxSimLogits(torch.autograd.Function):
    """compute_colbert_similarity (reference loss.py:20-46) without ever holding the [Nt, Ni, n, q] tensor of the
    reference's einsum: per chunk of text samples the similarities S[(m,n), (k,q)] are one GEMM of the flattened token
    matrices (bf16 MFMA NT kernel for bf16 tokens, exact-fp32 kernel for fp32), reduced at once to the per-(m,n,k)
    maximum + arg-max and the masked mean.  Backward rebuilds the sparse d(S) from the arg-max and reuses the dgrad /
    wgrad GEMMs.  Returns logits_per_text_token [Nt, Ni] (unscaled)."""

    @staticmethod
    def forward(ctx, tok_img, tok_txt):
        ni, q, e = tok_img.shape
        nt, n, _ = tok_txt.shape
        dt = tok_txt.dtype
        assert tok_img.dtype == dt and dt in (torch.float32, torch.bfloat16)
        if dt == torch.bfloat16 and ((ni * q) % 8 or (nt * n) % 8 or nt % 8 or e % 8):
            raise ValueError("bf16 MaxSim needs the text batch, (image batch x image tokens) and the embed dim to be "
                             "multiples of 8 (GEMM alignment); use fp32 token features otherwise")
        img = tok_img.contiguous().view(ni * q, e)
        txt = tok_txt.contiguous().view(nt * n, e)
        esz = 4 if dt == torch.float32 else 2
        ct = max(1, min(nt, ops.MAXSIM_GENERAL_BYTES // max(1, n * ni * q * esz)))
        if dt == torch.bfloat16:
            ct = max(8, ct // 8 * 8) if nt >= 8 else nt
        logits = torch.empty((nt, ni), dtype=torch.float32, device=img.device)
        inv_count = torch.empty((nt, ni), dtype=torch.float32, device=img.device)
        arg = torch.empty((nt * n, ni), dtype=torch.uint8, device=img.device)
        for m0 in range(0, nt, ct):
            m1 = min(nt, m0 + ct)
            rows = (m1 - m0) * n
            xt = txt[m0 * n:m1 * n]
            if dt == torch.float32:
                S = torch.empty((rows, ni * q), dtype=torch.float32, device=img.device)
                ops.gemm_f32(rows, ni * q, e, xt, e, 1, img, 1, e, S, ni * q)
            else:
                S = ops.linear_fwd(xt, img, None)
            maxv, a = ops.maxsim_reduce(S, q)
            del S
            lg, inv = ops.masked_mean(maxv, m1 - m0, n)
            logits[m0:m1] = lg
            inv_count[m0:m1] = inv
            arg[m0 * n:m1 * n] = a
        ctx.save_for_backward(img, txt, inv_count, arg)
        ctx.dims = (ni, q, nt, n, e, ct)
        return logits

    @staticmethod
    def backward(ctx, dlogits):
        img, txt, inv_count, arg = ctx.saved_tensors
        ni, q, nt, n, e, ct = ctx.dims
        dt = txt.dtype
        dlogits = dlogits.contiguous().float()
        dimg = torch.empty((ni * q, e), dtype=torch.float32, device=img.device)
        dtxt = torch.empty((nt * n, e), dtype=torch.float32, device=img.device)
        ws = img_t = None
        if dt == torch.bfloat16:
            ws = torch.empty((max(ops.linear_wgrad_ws_bytes(dt, ct * n, ni * q, e), 16),), dtype=torch.uint8, device=img.device)
            # [E, Ni*q] copy of the image tokens: dText = P @ img is then an NT GEMM like every dgrad
            img16 = torch.empty_like(img)
            img_t = torch.empty((e, ni * q), dtype=torch.bfloat16, device=img.device)
            ops.cast_weight(img.float(), img16, img_t)
        for m0 in range(0, nt, ct):
            m1 = min(nt, m0 + ct)
            rows = (m1 - m0) * n
            xt = txt[m0 * n:m1 * n]
            P, _ = ops.maxsim_scatter(dlogits[m0:m1], inv_count[m0:m1], arg[m0 * n:m1 * n], n, q, dt, False)
            beta = 0.0 if m0 == 0 else 1.0
            if dt == torch.float32:
                ops.gemm_f32(rows, e, ni * q, P, ni * q, 1, img, e, 1, dtxt[m0 * n:m1 * n], e)              # P @ img
                ops.gemm_f32(ni * q, e, rows, P, 1, ni * q, xt, e, 1, dimg, e, 1.0, beta)                    # P^T @ txt
            else:
                ops.linear_fwd(P, img_t, None, out=dtxt[m0 * n:m1 * n], out_dtype=torch.float32)   # P @ img
                ops.linear_wgrad(P, xt, dimg, beta, ws)                                           # P^T @ txt
        return dimg.view(ni, q, e).to(dt), dtxt.view(nt, n, e).to(dt)


class _MaxSimFused(torch.autograd.Function):
    """compute_colbert_similarity for bf16 token features with >= 16 tokens per image -- the fork's own operating points
    (ViT-B-16-colxlip: 196 image tokens, ViT-B-32-colxlip: 49; reference src/colxlip.sh: 512 pairs per GPU, global logits on
    every rank) -- with
    neither the [Nt, Ni, n, q] tensor of the reference's einsum nor the [Nt n, Ni q] similarity matrix of `_MaxSimLogits` in
    memory (csrc/colbert.hip "Fused MaxSim", csrc/gemm_nt_maxsim.h):
      * trailing text positions of a sample that are bitwise equal to its last position -- every position at or behind the EOT
        leaves ColXLIP's token head as the same vector (reference model.py:589-603) -- are computed ONCE and weighted by their
        count in the masked mean: same values, same non-zero count, the gradient of the representative copied to each of them;
      * the similarity GEMM's epilogue keeps per-(row, image) maxima + first arg-max instead of writing S;
      * backward: d(S) is rebuilt on the packed rows from arg-max and 1/count, dText = P img, dImg = P^T (w . text) on the
        NT / TN GEMM kernels.
    One 4-byte device-to-host read (the packed row count sizes the launches)."""

    P_CHUNK_BYTES = 8 << 30        # d(S) of the backward.  Sized for 288 GB: dText = P img has only E / 256 = 2 tile columns, so a chunk needs
                                   # >= 16.5 k rows to fill the chip with 256x256 tiles (below that the GEMM falls to the 128-row
                                   # one-barrier kernel, 0.75x); 4.5 GB at N = 512 -- one chunk

    @staticmethod
    def applies(tok_img, tok_txt) -> bool:
        ni, q, _ = tok_img.shape
        return ops.maxsim_fused_applies(tok_img, tok_txt) and (ni * q) % 8 == 0

    @staticmethod
    def forward(ctx, tok_img, tok_txt):
        ni, q, e = tok_img.shape
        nt, n, _ = tok_txt.shape
        img = tok_img.contiguous().view(ni * q, e)
        txt = tok_txt.contiguous()
        dev = img.device
        cu, R = ops.maxsim_pack_text(txt)
        packed, row_m, row_w = ops.maxsim_pack_rows(txt, cu, R)
        ld = (R + 255) // 256 * 256
        prow = ops.maxsim_partial_rows(ni, q)
        maxvT = torch.empty((ni, ld), dtype=torch.float32, device=dev)
        argT = torch.empty((ni, ld), dtype=torch.int16, device=dev)
        # partial maxima: 6 bytes per (row, slot, segment) -- per (row, image, slot half) below 64 tokens per image; rows in
        # chunks when that would pass ops.MAXSIM_PARTIAL_BYTES
        rows_per = max(256, (ops.MAXSIM_PARTIAL_BYTES // (6 * prow)) // 256 * 256)
        for r0 in range(0, R, rows_per):
            rc = min(rows_per, R - r0)
            ldp = (rc + 255) // 256 * 256
            pmax = torch.empty((prow, ldp), dtype=torch.float32, device=dev)
            pidx = torch.empty((prow, ldp), dtype=torch.int16, device=dev)
            ops.maxsim_gemm(packed[r0:r0 + rc], img, ni, q, pmax, pidx, ldp)
            ops.maxsim_finish(rc, ldp, r0, ld, ni, q, pmax, pidx, maxvT, argT)
            del pmax, pidx
        logits, inv_count = ops.maxsim_mean(nt, ni, ld, cu, row_w, maxvT)
        ctx.save_for_backward(img, packed, row_m, row_w, cu, inv_count, argT)
        ctx.dims = (ni, q, nt, n, e, R, ld)
        return logits

    @staticmethod
    def backward(ctx, dlogits):
        img, packed, row_m, row_w, cu, inv_count, argT = ctx.saved_tensors
        ni, q, nt, n, e, R, ld = ctx.dims
        dev = img.device
        dlogits = dlogits.contiguous().float()
        dimg = torch.empty((ni * q, e), dtype=torch.float32, device=dev)
        dpacked = torch.empty((R, e), dtype=torch.float32, device=dev)
        # [E, Ni q] copy of the image tokens: dText = P @ img is then an NT GEMM like every dgrad
        img16 = torch.empty_like(img)
        img_t = torch.empty((e, ni * q), dtype=torch.bfloat16, device=dev)
        ops.cast_weight(img.float(), img16, img_t)
        del img16
        packed_w = ops.maxsim_scale_rows(packed, row_w)          # a representative row stands for row_w original positions
        rows_per = max(256, (_MaxSimFused.P_CHUNK_BYTES // (2 * ni * q)) // 256 * 256)
        ws = torch.empty((max(ops.linear_wgrad_ws_bytes(torch.bfloat16, min(rows_per, R), ni * q, e), 16),), dtype=torch.uint8, device=dev)
        for r0 in range(0, R, rows_per):
            rc = min(rows_per, R - r0)
            P = torch.empty((rc, ni * q), dtype=torch.bfloat16, device=dev)
            ops.maxsim_scatter_packed(rc, r0, ld, ni, q, row_m, dlogits, inv_count, argT, P)
            # P @ img, bf16 out (what the returned gradient is rounded to anyway): the ping-pong NT kernel takes it, the fp32-output
            # form runs on the one-barrier kernel (0.7x)
            ops.cast_bf16_f32(ops.linear_fwd(P, img_t, None), dpacked[r0:r0 + rc])
            # P^T @ (w . text).  The ping-pong TN kernel addresses an operand through one 2-GiB buffer descriptor: row blocks of
            # P below that (the one-barrier kernel that takes larger ones runs at 0.7x)
            sub = max(256, ((1 << 31) - 1) // (2 * ni * q) // 256 * 256)
            for s0 in range(0, rc, sub):
                s1 = min(rc, s0 + sub)
                ops.linear_wgrad(P[s0:s1], packed_w[r0 + s0:r0 + s1], dimg, 0.0 if (r0 == 0 and s0 == 0) else 1.0, ws)
            del P
        dtxt = ops.maxsim_expand(dpacked, cu, nt, n, torch.bfloat16)
        return dimg.view(ni, q, e).to(torch.bfloat16), dtxt


class _SymmetricCEOfLogits(torch.autograd.Function):
    """0.5/N * (sum_r CE(z[r,:], r) + sum_c CE(z[:,c], c)) with z = scale * raw (loss.py:285-288 on given logits)."""

    @staticmethod
    def forward(ctx, raw, scale):
        raw = raw.contiguous().float()
        scale = scale.detach().float().reshape(1).contiguous()
        r, c = raw.shape
        assert r == c
        z = ops.scale_by_dev(raw, scale)
        w = 0.5 / r
        loss = torch.zeros((1,), dtype=torch.float32, device=raw.device)
        lse_r = torch.empty((r,), dtype=torch.float32, device=raw.device)
        lse_c = torch.empty((c,), dtype=torch.float32, device=raw.device)
        ops.ce_rows(z, 0, lse_r, w, loss)
        ops.ce_cols(z, lse_c, w, loss)
        ctx.save_for_backward(z, lse_r, lse_c, scale)
        ctx.w = w
        return loss.reshape(())

    @staticmethod
    def backward(ctx, gout):
        z, lse_r, lse_c, scale = ctx.saved_tensors
        dscale = torch.zeros((1,), dtype=torch.float32, device=z.device)
        ops.ce_grad(z, 0, lse_r, ctx.w, lse_c, ctx.w, scale, dscale)          # z -> dz in place
        gout = gout.reshape(1).float()
        draw = ops.scale_by_dev(z, scale * gout, out=z) if ctx.needs_input_grad[0] else None
        ds = (dscale * gout).reshape(()) if ctx.needs_input_grad[1] else None
        return draw, ds


class _RowBlockSymmetricCE(torch.autograd.Function):
    """The symmetric cross-entropy of ColClipLoss's token logits when every rank holds only ITS rows of the [N, N] matrix
    (`ColClipLoss(rows_local=True)`): raw [b, N] = this rank's b text samples against all N images, label of row m = off + m.

        loss_rank = 1/(2b) * ( sum_m (lse_row[m] - z[m, off+m])  +  sum_{k in this rank's columns} (lse_col[k] - z[k-off, k]) )

    with lse_col the column log-sum-exps over ALL ranks' rows: each rank reduces its own rows (one pass over its block), the
    [W, N] partials are all-gathered (N floats per rank) and folded.  The mean over ranks of loss_rank is the global loss the
    reference computes on every rank (loss.py:259-296); this is ClipLoss's `local_loss` convention (loss.py:119-130,144-146)
    applied to the token term.  Backward by formula, not through the collective: dz[m, k] = 1/(2b) * (softmax_row - [k == off+m]
    + exp(z - lse_col[k]) - [k == off+m]) for the rank's rows and ALL columns -- the part of sum_ranks loss_rank that depends on
    this rank's rows."""

    @staticmethod
    def forward(ctx, raw, scale, off: int, world_size: int):
        raw = raw.contiguous().float()
        scale = scale.detach().float().reshape(1).contiguous()
        b, n = raw.shape
        z = ops.scale_by_dev(raw, scale)
        w = 0.5 / b
        loss = torch.zeros((1,), dtype=torch.float32, device=raw.device)
        lse_r = torch.empty((b,), dtype=torch.float32, device=raw.device)
        part = torch.empty((n,), dtype=torch.float32, device=raw.device)
        sink = torch.zeros((1,), dtype=torch.float32, device=raw.device)
        ops.ce_rows(z, off, lse_r, w, loss)
        ops.ce_cols(z, part, 0.0, sink)                      # log-sum-exp of every column over THIS rank's rows
        allp = torch.empty((world_size * n,), dtype=torch.float32, device=raw.device)
        with torch.no_grad():
            dist.all_gather_into_tensor(allp, part)
        lse_c = torch.logsumexp(allp.view(world_size, n), dim=0)     # [N]: glue on W x N floats
        idx = torch.arange(b, device=raw.device)
        loss = loss + w * (lse_c[off:off + b] - z[idx, off + idx]).sum()
        ctx.save_for_backward(z, lse_r, lse_c, scale)
        ctx.w, ctx.off = w, off
        return loss.reshape(())

    @staticmethod
    def backward(ctx, gout):
        z, lse_r, lse_c, scale = ctx.saved_tensors
        dscale = torch.zeros((1,), dtype=torch.float32, device=z.device)
        ops.ce_grad(z, ctx.off, lse_r, ctx.w, lse_c, ctx.w, scale, dscale, col_label_off=ctx.off)      # z -> dz in place
        gout = gout.reshape(1).float()
        draw = ops.scale_by_dev(z, scale * gout, out=z) if ctx.needs_input_grad[0] else None
        ds = (dscale * gout).reshape(()) if ctx.needs_input_grad[1] else None
        return draw, ds, None, None


def compute_colbert_similarity(token_image_features, token_text_features):
    """reference loss.py:20-46 -> [batch_txt, batch_img]."""
    if _MaxSimFused.applies(token_image_features, token_text_features):
        return _MaxSimFused.apply(token_image_features, token_text_features)
    return _MaxSimLogits.apply(token_image_features, token_text_features)


class ColClipLoss(nn.Module):
    """reference loss.py:184-296: alpha * global CLIP loss + (1 - alpha) * the same loss on MaxSim token logits."""

    def __init__(self, local_loss=False, gather_with_grad=False, cache_labels=False, rank=0, world_size=1,
                 use_horovod=False, alpha=0.5, rows_local=False, **kwargs):
        super().__init__()
        # EXTENSION (not in the reference, which computes the global [N, N] token logits on EVERY rank and refuses local_loss,
        # loss.py:246-256): `rows_local=True` has each rank compute only its own text rows against all images -- MaxSim on [b, N]
        # instead of [N, N], 1/W of the loss work, no gather of the text tokens -- with the column statistics exchanged as N
        # floats per rank.  Needs gather_with_grad (the image-token gradients of the other ranks' rows arrive through the
        # gather's reduce-scatter).  The mean over ranks of the returned losses is the reference's global loss, and with
        # gather_with_grad every leaf receives the gradient the reference run delivers (tests/test_two_ranks_gpu.py against
        # tests/golden/colclip_dist.npz).  At the fork's own launch point (src/colxlip.sh: 4 x 512) the global form is 16 MaxSim
        # blocks of 512 x 512 per rank, this one 4.
        self.rows_local = bool(rows_local)
        if self.rows_local and world_size > 1 and not gather_with_grad:
            raise ValueError("ColClipLoss(rows_local=True) needs gather_with_grad=True: a rank's image tokens receive gradient from "
                             "every rank's text rows")
        self.local_loss = local_loss
        self.gather_with_grad = gather_with_grad
        self.cache_labels = cache_labels
        self.rank = rank
        self.world_size = world_size
        self.use_horovod = use_horovod
        self.alpha = alpha
        self.prev_num_logits = 0
        self.labels = {}

    get_ground_truth = ClipLoss.get_ground_truth

    def _gather_all(self, image_features, text_features, token_image_features, token_text_features):
        if self.world_size > 1:
            if self.local_loss:
                raise NotImplementedError          # as the reference (loss.py:246-248)
            kw = dict(local_loss=self.local_loss, gather_with_grad=self.gather_with_grad, rank=self.rank,
                      world_size=self.world_size, use_horovod=self.use_horovod)
            image_features, text_features = gather_features(image_features, text_features, **kw)
            token_image_features, token_text_features = gather_features(token_image_features, token_text_features, **kw)
        return image_features, text_features, token_image_features, token_text_features

    def get_logits(self, image_features, text_features, token_image_features, token_text_features, logit_scale,
                   logit_bias=None):
        fi, ft, ti, tt = self._gather_all(image_features, text_features, token_image_features, token_text_features)
        logits_per_image = _ScaledMatmul.apply(fi, ft, logit_scale)
        logits_per_text = logits_per_image.T
        logits_per_text_token = logit_scale * compute_colbert_similarity(ti, tt)
        logits_per_image_token = logits_per_text_token.T
        if logit_bias is not None:
            logits_per_image = logits_per_image + logit_bias
            logits_per_text = logits_per_text + logit_bias
        return {"logits_per_image": logits_per_image, "logits_per_text": logits_per_text,
                "logits_per_image_token": logits_per_image_token, "logits_per_text_token": logits_per_text_token}

    def _forward_rows_local(self, image_features, text_features, token_image_features, token_text_features, logit_scale, output_dict):
        W, rank = self.world_size, self.rank
        b = image_features.shape[0]
        off = b * rank
        all_fi = _AllGatherCat.apply(image_features, rank, W)
        all_ft = _AllGatherCat.apply(text_features, rank, W)
        global_contrastive_loss = (contrastive_ce(image_features, all_ft, logit_scale, off, False) +
                                   contrastive_ce(text_features, all_fi, logit_scale, off, False))
        all_ti = _AllGatherCat.apply(token_image_features, rank, W)
        raw = compute_colbert_similarity(all_ti, token_text_features)              # [b, N]: this rank's text rows
        token_contrastive_loss = _RowBlockSymmetricCE.apply(raw, logit_scale, off, W)
        total_loss = self.alpha * global_contrastive_loss + (1 - self.alpha) * token_contrastive_loss
        if output_dict:
            return {"global_contrastive_loss": global_contrastive_loss, "token_contrastive_loss": token_contrastive_loss,
                    "total_loss": total_loss}
        return total_loss

    def forward(self, image_features=None, text_features=None, token_image_features=None, token_text_features=None,
                logit_scale=None, logit_bias=None, output_dict=False, **kwargs):
        if self.rows_local and self.world_size > 1:
            return self._forward_rows_local(image_features, text_features, token_image_features, token_text_features, logit_scale,
                                            output_dict)
        fi, ft, ti, tt = self._gather_all(image_features, text_features, token_image_features, token_text_features)
        global_contrastive_loss = contrastive_ce(fi, ft, logit_scale, 0, True)
        token_contrastive_loss = _SymmetricCEOfLogits.apply(compute_colbert_similarity(ti, tt), logit_scale)
        total_loss = self.alpha * global_contrastive_loss + (1 - self.alpha) * token_contrastive_loss
        if output_dict:
            return {"global_contrastive_loss": global_contrastive_loss, "token_contrastive_loss": token_contrastive_loss,
                    "total_loss": total_loss}
        return total_loss


# --------------------------------------------------------------------------- SigLipLoss (reference loss.py:396-604)
def _exchange_post(sends, recvs, group=None):
    """Post one round of point-to-point transfers: sends [(tensor, to_rank)], recvs [(from_rank, like_tensor)].  Returns a
    callable that waits and hands back the received device tensors in `recvs` order.  RCCL moves device tensors with
    batch_isend_irecv; gloo stages them through host memory (its P2P on device tensors is not relied on)."""
    from .distributed import backend_is_rccl
    if backend_is_rccl(group):
        out = [torch.empty_like(like) for _, like in recvs]
        ops_ = [dist.P2POp(dist.isend, t.contiguous(), to, group=group) for t, to in sends]
        ops_ += [dist.P2POp(dist.irecv, o, frm, group=group) for o, (frm, _) in zip(out, recvs)]
        reqs = dist.batch_isend_irecv(ops_)

        def wait():
            for req in reqs:
                req.wait()
            return out
        return wait
    host_out = [torch.empty(like.shape, dtype=like.dtype) for _, like in recvs]
    host_in = [t.detach().contiguous().cpu() for t, _ in sends]
    reqs = [dist.isend(h, to, group=group) for h, (_, to) in zip(host_in, sends)]
    reqs += [dist.irecv(h, frm, group=group) for h, (frm, _) in zip(host_out, recvs)]
    devices = [like.device for _, like in recvs]

    def wait():
        for req in reqs:
            req.wait()
        return [h.to(d) for h, d in zip(host_out, devices)]
    return wait


def neighbour_exchange(from_rank, to_rank, tensor, group=None):
    """reference loss.py:396-410: send `tensor` to `to_rank`, receive the same shape from `from_rank`."""
    return _exchange_post([(tensor, to_rank)], [(from_rank, tensor)], group)()[0]


def neighbour_exchange_bidir(left_rank, right_rank, tensor_to_left, tensor_to_right, group=None):
    """reference loss.py:413-432: returns (tensor_from_right, tensor_from_left)."""
    got = _exchange_post([(tensor_to_left, left_rank), (tensor_to_right, right_rank)],
                         [(right_rank, tensor_to_left), (left_rank, tensor_to_right)], group)()
    return got[0], got[1]


class NeighbourExchange(torch.autograd.Function):
    """reference loss.py:435-446: the gradient goes back to the rank the tensor came from."""

    @staticmethod
    def forward(ctx, from_rank, to_rank, group, tensor):
        ctx.group, ctx.from_rank, ctx.to_rank = group, from_rank, to_rank
        return neighbour_exchange(from_rank, to_rank, tensor, group=group)

    @staticmethod
    def backward(ctx, grad_output):
        return (None, None, None) + (NeighbourExchange.apply(ctx.to_rank, ctx.from_rank, ctx.group, grad_output),)


def neighbour_exchange_with_grad(from_rank, to_rank, tensor, group=None):
    return NeighbourExchange.apply(from_rank, to_rank, group, tensor)


class NeighbourExchangeBidir(torch.autograd.Function):
    """reference loss.py:453-464."""

    @staticmethod
    def forward(ctx, left_rank, right_rank, group, tensor_to_left, tensor_to_right):
        ctx.group, ctx.left_rank, ctx.right_rank = group, left_rank, right_rank
        return neighbour_exchange_bidir(left_rank, right_rank, tensor_to_left, tensor_to_right, group=group)

    @staticmethod
    def backward(ctx, *grad_outputs):
        return (None, None, None) + NeighbourExchangeBidir.apply(ctx.right_rank, ctx.left_rank, ctx.group, *grad_outputs)


def neighbour_exchange_bidir_with_grad(left_rank, right_rank, tensor_to_left, tensor_to_right, group=None):
    return NeighbourExchangeBidir.apply(left_rank, right_rank, group, tensor_to_left, tensor_to_right)


def _ring_rounds(rank, world_size, impl):
    """The reference's exchange pattern (loss.py:527-584) as rounds of lanes (source block, to_rank, from_rank); block 0 is
    this rank's own text features, every lane of a round appends the block it receives."""
    right, left = (rank + 1) % world_size, (rank - 1 + world_size) % world_size
    rounds = []
    if impl == "shift":
        for k in range(world_size - 1):
            rounds.append([(k, right, left)])
        return rounds
    to_left = to_right = 0
    num_bidir, remainder = divmod(world_size - 1, 2)
    n = 1
    for _ in range(num_bidir):
        rounds.append([(to_left, left, right), (to_right, right, left)])   # receives (from_right, from_left)
        to_left, to_right = n, n + 1
        n += 2
    if remainder:
        rounds.append([(to_right, right, left)])
    return rounds


class _SigmoidBlocks:
    """The per-block kernels: loss of z = scale * a @ blk.T + bias over one text block, with (fused dims) dA formed in the
    forward walk or (other dims) the d(logits) matrix kept for the backward GEMMs."""

    def __init__(self, a, scale, bias, inv_r, want_grad):
        self.a, self.scale, self.bias, self.inv_r, self.want = a, scale, bias, inv_r, want_grad
        self.fused = a.shape[1] in ops.FUSED_CE_DIMS
        self.out3 = None
        self.dA = None
        self.dz = []                       # dense: d(logits) of every block, in forward order

    def forward(self, blk, pos_off):
        if self.fused:
            self.out3, self.dA = ops.sigmoid_fused_fwd(self.a, blk, self.scale, self.bias, pos_off, self.inv_r, self.want,
                                                       out3=self.out3, dA=self.dA)
            return
        r, e = self.a.shape
        c = blk.shape[0]
        z = torch.empty((r, c), dtype=torch.float32, device=self.a.device)
        ops.gemm_f32(r, c, e, self.a, e, 1, blk, 1, e, z, c)
        o3 = ops.sigmoid_dense(z, self.scale, self.bias, pos_off, self.inv_r)
        self.out3 = o3 if self.out3 is None else self.out3 + o3
        if self.want:
            self.dz.append(z)

    def grad_a(self, blocks, gout):
        """dA * upstream (dense: every block's d(logits) @ block, scaled by scale * upstream)"""
        if self.fused:
            return ops.scale_by_dev(self.dA, gout)
        r, e = self.a.shape
        sg = self.scale * gout
        da = torch.empty((r, e), dtype=torch.float32, device=self.a.device)
        for i, (z, blk) in enumerate(zip(self.dz, blocks)):
            ops.scale_by_dev(z, sg, out=z)
            ops.gemm_f32(r, e, blk.shape[0], z, blk.shape[0], 1, blk, e, 1, da, e, 1.0, 0.0 if i == 0 else 1.0)
        return da

    def grad_block(self, i, blk, pos_off, gout, out=None):
        """d(block i) * upstream; added to `out` when given.  Dense: after grad_a (the block's d(logits) already scaled)."""
        if self.fused:
            return ops.sigmoid_fused_bwd(self.a, blk, self.scale, self.bias, pos_off, self.inv_r, gout, dB=out,
                                         accumulate=out is not None)
        r, e = self.a.shape
        c = blk.shape[0]
        dst = out if out is not None else torch.empty((c, e), dtype=torch.float32, device=self.a.device)
        ops.gemm_f32(c, e, r, self.dz[i], 1, c, self.a, e, 1, dst, e, 1.0, 1.0 if out is not None else 0.0)
        return dst


def _prep(a, b, scale, bias):
    a = a.contiguous().float()
    b = b.contiguous().float()
    return a, b, scale.detach().float().reshape(1).contiguous(), bias.detach().float().reshape(1).contiguous()


class _SigmoidLoss(torch.autograd.Function):
    """SigLIP loss of one block: 1/r * sum softplus(-y z), z = scale * a @ b.T + bias, positives at column row + pos_off
    (pos_off < 0: none).  The W == 1 case, and the gathered [b, W*b] block of dist_impl gather / reduce."""

    @staticmethod
    def forward(ctx, a, b, scale, bias, pos_off: int, want_grad: bool):
        with phase("loss.fwd"):
            a, b, s, bi = _prep(a, b, scale, bias)
            k = _SigmoidBlocks(a, s, bi, 1.0 / a.shape[0], want_grad)
            k.forward(b, pos_off)
        ctx.k, ctx.b, ctx.pos_off = k, b, pos_off
        ctx.shapes = (scale.shape, bias.shape)
        return k.out3[0].clone().reshape(())

    @staticmethod
    def backward(ctx, gout):
        k, b = ctx.k, ctx.b
        with phase("loss.bwd"):
            gout = gout.reshape(1).float().contiguous()
            da = k.grad_a([b], gout)
            db = k.grad_block(0, b, ctx.pos_off, gout) if ctx.needs_input_grad[1] else None
            g2 = ops.scale_by_dev(k.out3[1:3].contiguous(), gout)
        ctx.k = ctx.b = None
        return (da if ctx.needs_input_grad[0] else None, db, g2[0].reshape(ctx.shapes[0]), g2[1].reshape(ctx.shapes[1]),
                None, None)


class _SigmoidRing(torch.autograd.Function):
    """SigLIP loss with the text blocks passed around the ring (dist_impl shift / bidir, reference loss.py:524-570): the
    next round's exchange is posted before the kernels on the current blocks run.  Backward: every received block's gradient
    travels back along the path it came by, the next round's kernels running while it is in flight."""

    @staticmethod
    def forward(ctx, a, b, scale, bias, rank: int, world_size: int, impl: str, want_grad: bool):
        a, b, s, bi = _prep(a, b, scale, bias)
        rounds = _ring_rounds(rank, world_size, impl)
        k = _SigmoidBlocks(a, s, bi, 1.0 / a.shape[0], want_grad)
        blocks = [b]
        with phase("loss.fwd"):
            pending = _exchange_post([(blocks[src], to) for src, to, _ in rounds[0]], [(frm, b) for _, _, frm in rounds[0]])
            k.forward(b, 0)
            for j in range(len(rounds)):
                got = pending()
                blocks += got
                if j + 1 < len(rounds):
                    pending = _exchange_post([(blocks[src], to) for src, to, _ in rounds[j + 1]],
                                             [(frm, b) for _, _, frm in rounds[j + 1]])
                for blk in got:
                    k.forward(blk, -1)
        ctx.k, ctx.blocks, ctx.rounds = k, blocks, rounds
        ctx.shapes = (scale.shape, bias.shape)
        return k.out3[0].clone().reshape(())

    @staticmethod
    def backward(ctx, gout):
        k, blocks, rounds = ctx.k, ctx.blocks, ctx.rounds
        with phase("loss.bwd"):
            gout = gout.reshape(1).float().contiguous()
            da = k.grad_a(blocks, gout)
            g = [None] * len(blocks)
            # block index received by each lane of each round
            recv_idx, n = [], 1
            for lanes in rounds:
                recv_idx.append(list(range(n, n + len(lanes))))
                n += len(lanes)
            pending, pend_lanes = None, None
            for j in range(len(rounds) - 1, -1, -1):
                for i in recv_idx[j]:                          # this round's received blocks (the sources of round j+1)
                    g[i] = k.grad_block(i, blocks[i], -1, gout, out=g[i])
                if pending is not None:
                    for (src, _, _), t in zip(pend_lanes, pending()):
                        g[src].add_(t)
                # the gradient of every block received in round j goes back to its sender; what this rank sent comes back
                pending = _exchange_post([(g[i], frm) for i, (_, _, frm) in zip(recv_idx[j], rounds[j])],
                                         [(to, blocks[0]) for _, to, _ in rounds[j]])
                pend_lanes = rounds[j]
            g[0] = k.grad_block(0, blocks[0], 0, gout, out=g[0])
            if pending is not None:
                for (src, _, _), t in zip(pend_lanes, pending()):
                    g[src].add_(t)
            g2 = ops.scale_by_dev(k.out3[1:3].contiguous(), gout)
        ctx.k = ctx.blocks = None
        return da, g[0], g2[0].reshape(ctx.shapes[0]), g2[1].reshape(ctx.shapes[1]), None, None, None, None


class SigLipLoss(nn.Module):
    """Sigmoid Loss for Language Image Pre-Training (SigLIP) - https://arxiv.org/abs/2303.15343 (reference loss.py:470-604).

    The loss runs in csrc/loss_sigmoid.hip (exact fp32, the logits recomputed tile by tile, 4 logits-GEMM equivalents per step).
    dist_impl: `gather` / `reduce` all-gather the text features once (backward: reduce-scatter) and run ONE launch over the
    [b, W*b] block with the positives at column rank*b -- the reference's sum of W block losses; `shift` / `bidir` pass the
    text blocks around the ring with one launch per received block."""

    def __init__(
            self,
            cache_labels: bool = False,
            rank: int = 0,
            world_size: int = 1,
            dist_impl: Optional[str] = None,
    ):
        super().__init__()
        self.cache_labels = cache_labels
        self.rank = rank
        self.world_size = world_size
        self.dist_impl = dist_impl or 'bidir'  # default to bidir exchange, as the reference
        assert self.dist_impl in ('bidir', 'shift', 'reduce', 'gather')

        # cache state (unused, as in the reference)
        self.prev_num_logits = 0
        self.labels = {}

    def get_ground_truth(self, device, dtype, num_logits, negative_only=False) -> torch.Tensor:
        """The dense label matrix (API surface; the loss itself never forms it)."""
        labels = -torch.ones((num_logits, num_logits), device=device, dtype=dtype)
        if not negative_only:
            labels = 2 * torch.eye(num_logits, device=device, dtype=dtype) + labels
        return labels

    def get_logits(self, image_features, text_features, logit_scale, logit_bias=None):
        logits = _ScaledMatmul.apply(image_features, text_features, logit_scale)
        if logit_bias is not None:
            logits = logits + logit_bias
        return logits

    def _loss(self, image_features, text_features, logit_scale, logit_bias=None, negative_only=False):
        if logit_bias is None:
            logit_bias = torch.zeros((), dtype=torch.float32, device=image_features.device)
        return _SigmoidLoss.apply(image_features, text_features, logit_scale, logit_bias, -1 if negative_only else 0,
                                  self._want_grad(image_features, text_features, logit_scale, logit_bias))

    @staticmethod
    def _want_grad(*ts):
        return torch.is_grad_enabled() and any(t.requires_grad for t in ts)

    def forward(self, image_features, text_features, logit_scale, logit_bias, output_dict=False):
        W = self.world_size
        want = self._want_grad(image_features, text_features, logit_scale, logit_bias)
        if W == 1:
            loss = _SigmoidLoss.apply(image_features, text_features, logit_scale, logit_bias, 0, want)
        elif self.dist_impl in ("gather", "reduce"):
            b = image_features.shape[0]
            all_text = _AllGatherCat.apply(text_features, self.rank, W) if want else _all_gather_nograd(text_features, W)
            loss = _SigmoidLoss.apply(image_features, all_text, logit_scale, logit_bias, self.rank * b, want)
        else:
            loss = _SigmoidRing.apply(image_features, text_features, logit_scale, logit_bias, self.rank, W, self.dist_impl, want)
        return {"contrastive_loss": loss} if output_dict else loss


# --------------------------------------------------------------------------- DistillClipLoss (reference loss.py:343-379)
def _prep_scaled(a, scale):
    a = a.contiguous().float()
    scale = scale.detach().float().reshape(1).contiguous()
    return a, scale, ops.scale_by_dev(a, scale)


class _DistillCE(torch.autograd.Function):
    """(contrastive, distill) of one problem: s = (scale*a) @ b.T (student), t = (tscale*ta) @ tb.T (teacher),
    contrastive = w * sum_r CE(s[r,:], r + off), distill = w * sum_r -(softmax(t[r,:]) * log_softmax(s[r,:])).sum()
    [+ the same over columns when symmetric], w = 0.5 / rows.

    Neither logits matrix is ever written to memory (csrc/loss_distill.hip): the forward keeps per-tile statistics of both,
    the backward recomputes both tiles per student operand.  The teacher gets no gradient here (distill_ce routes a teacher
    that needs one to _DistillCEDense)."""

    @staticmethod
    def forward(ctx, a, b, scale, ta, tb, tscale, label_off: int, symmetric: bool):
        with phase("loss.fwd"):
            a, scale, a_s = _prep_scaled(a, scale)
            b = b.contiguous().float()
            _, tscale, ta_s = _prep_scaled(ta, tscale)
            tb = tb.contiguous().float()
            r = a.shape[0]
            if symmetric:
                assert r == b.shape[0] and label_off == 0
            w = 0.5 / r
            loss2 = torch.zeros((2,), dtype=torch.float32, device=a.device)
            st_r, st_c = ops.distill_fused_fwd(a_s, b, ta_s, tb, label_off, symmetric, w, w, loss2)
        ctx.save_for_backward(a_s, b, ta_s, tb, scale, st_r, st_c if st_c is not None else st_r)
        ctx.label_off, ctx.symmetric, ctx.w = label_off, symmetric, w
        return loss2[0].clone(), loss2[1].clone()

    @staticmethod
    def backward(ctx, gc, gd):
        a_s, b, ta_s, tb, scale, st_r, st_c = ctx.saved_tensors
        off, w = ctx.label_off, ctx.w
        st_c = st_c if ctx.symmetric else None
        with phase("loss.bwd"):
            gc = gc.reshape(1).float().contiguous()
            gd = gd.reshape(1).float().contiguous()
            need_a, need_b, need_s = ctx.needs_input_grad[0], ctx.needs_input_grad[1], ctx.needs_input_grad[2]
            da = db = ds = None
            dscale = torch.zeros((1,), dtype=torch.float32, device=a_s.device) if need_s else None
            if need_a or need_s:
                # rows of `a` own the walk: d(a) = scale * ds @ b; d(scale) = sum ds*s / scale rides along
                da = ops.distill_fused_bwd(a_s, b, ta_s, tb, st_r, w, off, st_c, w, 0, gc, gd, scale, dscale, scale)
                if not need_a:
                    da = None
            if need_b:
                # rows of `b` own the walk: d(b) = ds.T @ (scale*a), both tiles seen transposed
                db = ops.distill_fused_bwd(b, a_s, tb, ta_s, st_c, w, 0, st_r, w, off, gc, gd, None)
            if need_s:
                ds = dscale.reshape(())
        return da, db, ds, None, None, None, None, None


class _DistillCEDense(torch.autograd.Function):
    """The same two losses with both logits matrices in memory: embed dims the fused kernels are not instantiated for, and a
    teacher whose features or scale need a gradient (dt = -w * g_d * pi * (s - sum pi s), reference autograd of loss.py:345)."""

    @staticmethod
    def forward(ctx, a, b, scale, ta, tb, tscale, label_off: int, symmetric: bool):
        a, scale, a_s = _prep_scaled(a, scale)
        b = b.contiguous().float()
        _, tscale, ta_s = _prep_scaled(ta, tscale)
        tb = tb.contiguous().float()
        r, c = a.shape[0], b.shape[0]
        if symmetric:
            assert r == c and label_off == 0
        s = torch.empty((r, c), dtype=torch.float32, device=a.device)
        ops.gemm_f32(r, c, a.shape[1], a_s, a.shape[1], 1, b, 1, b.shape[1], s, c)
        t = torch.empty((r, c), dtype=torch.float32, device=a.device)
        ops.gemm_f32(r, c, ta.shape[1], ta_s, ta.shape[1], 1, tb, 1, tb.shape[1], t, c)
        w = 0.5 / r
        loss2 = torch.zeros((2,), dtype=torch.float32, device=a.device)
        st_r, st_c = ops.distill_dense_fwd(s, t, label_off, symmetric, w, w, loss2)
        ctx.save_for_backward(a_s, b, ta_s, tb, scale, tscale, s, t, st_r, st_c if st_c is not None else st_r)
        ctx.label_off, ctx.symmetric, ctx.w = label_off, symmetric, w
        return loss2[0].clone(), loss2[1].clone()

    @staticmethod
    def backward(ctx, gc, gd):
        a_s, b, ta_s, tb, scale, tscale, s, t, st_r, st_c = ctx.saved_tensors
        r, e = a_s.shape
        c, et = b.shape[0], ta_s.shape[1]
        gc = gc.reshape(1).float().contiguous()
        gd = gd.reshape(1).float().contiguous()
        want_t = any(ctx.needs_input_grad[3:6])
        dscales = torch.zeros((2,), dtype=torch.float32, device=s.device)
        # s -> ds and t -> dt in place (consumes the saved logits)
        ops.distill_dense_grad(s, t, ctx.label_off, st_r, ctx.w, st_c if ctx.symmetric else None, ctx.w, gc, gd, want_t,
                               scale, tscale if want_t else None, dscales)
        da = db = dta = dtb = None
        if ctx.needs_input_grad[0]:
            tmp = torch.empty((r, e), dtype=torch.float32, device=s.device)
            ops.gemm_f32(r, e, c, s, c, 1, b, e, 1, tmp, e)                 # ds @ b
            da = ops.scale_by_dev(tmp, scale, out=tmp)
        if ctx.needs_input_grad[1]:
            db = torch.empty((c, e), dtype=torch.float32, device=s.device)
            ops.gemm_f32(c, e, r, s, 1, c, a_s, e, 1, db, e)                # ds.T @ (scale*a)
        if ctx.needs_input_grad[3]:
            tmp = torch.empty((r, et), dtype=torch.float32, device=s.device)
            ops.gemm_f32(r, et, c, t, c, 1, tb, et, 1, tmp, et)             # dt @ tb
            dta = ops.scale_by_dev(tmp, tscale, out=tmp)
        if ctx.needs_input_grad[4]:
            dtb = torch.empty((c, et), dtype=torch.float32, device=s.device)
            ops.gemm_f32(c, et, r, t, 1, c, ta_s, et, 1, dtb, et)          # dt.T @ (tscale*ta)
        ds = dscales[0].reshape(()) if ctx.needs_input_grad[2] else None
        dts = dscales[1].reshape(()) if ctx.needs_input_grad[5] else None
        return da, db, ds, dta, dtb, dts, None, None


def distill_ce(a, b, scale, ta, tb, tscale, label_off: int, symmetric: bool):
    """(contrastive, distill) of one problem; the fused kernels unless an embed dim is outside ops.FUSED_CE_DIMS or the
    teacher needs a gradient."""
    teacher_grad = torch.is_grad_enabled() and any(x.requires_grad for x in (ta, tb, tscale))
    if not teacher_grad and a.shape[1] in ops.FUSED_CE_DIMS and ta.shape[1] in ops.FUSED_CE_DIMS:
        return _DistillCE.apply(a, b, scale, ta, tb, tscale, label_off, symmetric)
    return _DistillCEDense.apply(a, b, scale, ta, tb, tscale, label_off, symmetric)


class DistillClipLoss(ClipLoss):
    """reference loss.py:343-379: ClipLoss's contrastive term plus the cross-entropy of the student's logits against the
    teacher's softmax, in both directions.  One fused launch pair per problem yields both losses (csrc/loss_distill.hip); the
    teacher features are gathered like the student's (ClipLoss.get_logits gathers both pairs in the reference)."""

    def dist_loss(self, teacher_logits, student_logits):
        """reference loss.py:345 on materialised logits (API surface; forward never forms them)."""
        return -(teacher_logits.softmax(dim=1) * student_logits.log_softmax(dim=1)).sum(dim=1).mean(dim=0)

    def forward(
            self,
            image_features,
            text_features,
            logit_scale,
            dist_image_features,
            dist_text_features,
            dist_logit_scale,
            output_dict=False,
            **kwargs,
    ):
        # NB like the reference (loss.py:347-376) logit_bias is not applied.
        if not torch.is_tensor(dist_logit_scale):
            dist_logit_scale = torch.tensor(float(dist_logit_scale), device=logit_scale.device)
        if self.world_size > 1:
            all_image_features, all_text_features = self._gather(image_features, text_features)
            dist_all_image, dist_all_text = self._gather(dist_image_features, dist_text_features)
            if self.local_loss:
                off = image_features.shape[0] * self.rank
                c_i, d_i = distill_ce(image_features, all_text_features, logit_scale, dist_image_features, dist_all_text,
                                      dist_logit_scale, off, False)
                c_t, d_t = distill_ce(text_features, all_image_features, logit_scale, dist_text_features, dist_all_image,
                                      dist_logit_scale, off, False)
                contrastive_loss, distill_loss = c_i + c_t, d_i + d_t
            else:
                contrastive_loss, distill_loss = distill_ce(all_image_features, all_text_features, logit_scale, dist_all_image,
                                                            dist_all_text, dist_logit_scale, 0, True)
        else:
            contrastive_loss, distill_loss = distill_ce(image_features, text_features, logit_scale, dist_image_features,
                                                        dist_text_features, dist_logit_scale, 0, True)

        if output_dict:
            return {"contrastive_loss": contrastive_loss, "distill_loss": distill_loss}

        return contrastive_loss, distill_loss
