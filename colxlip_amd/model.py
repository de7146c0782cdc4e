"""CLIP model whose towers run on libclipx_hip.so.

Drop-in for the model object the reference's `create_model_and_transforms` returns
(reference factory.py:289 -> open_clip.model.CLIP; contract mirrored in the reference at
model.py:500-511,544-556,569-609,656-668): same state-dict keys and shapes,
`model(image, text) -> {"image_features","text_features","logit_scale"}`,
`.encode_image/.encode_text(x, normalize=)`, `.visual.image_size`, `.visual.preprocess_cfg`,
`.set_grad_checkpointing()`, `.logit_scale`, `.output_dict`.

Nothing here computes with PyTorch ops: the nn.Modules only own the fp32 master parameters;
each tower is ONE autograd.Function whose forward/backward enqueue hand-written HIP kernels
(patch-embed GEMM, LayerNorm, QKV/out/MLP GEMMs, fused attention, pooling, projection).
Precision: 'fp32' runs every kernel in exact fp32 (parity mode); everything else runs bf16
operands with fp32 accumulation/statistics and fp32 master weights (the reference's `bf16`
mode keeps bf16 masters and bf16 Adam moments; we deliberately keep fp32 masters).
"""
from __future__ import annotations

import copy
import math
import os
from dataclasses import dataclass
from typing import Any, Dict, List, Optional, Tuple, Union

import torch
from torch import nn

from . import ops
from .trace import phase
from ._lib import ACT_GELU, ACT_QUICKGELU


# --------------------------------------------------------------------------- configs (model.py:26-84)
@dataclass
class CLIPVisionCfg:
    layers: int = 12
    width: int = 768
    head_width: int = 64
    mlp_ratio: float = 4.0
    patch_size: int = 16
    image_size: Union[Tuple[int, int], int] = 224
    ls_init_value: Optional[float] = None
    patch_dropout: float = 0.0
    attentional_pool: bool = False
    no_ln_pre: bool = False
    pos_embed_type: str = "learnable"
    final_ln_after_pool: bool = False
    pool_type: str = "tok"
    output_tokens: bool = False
    act_kwargs: Optional[dict] = None
    norm_kwargs: Optional[dict] = None
    timm_model_name: Optional[str] = None


@dataclass
class CLIPTextCfg:
    context_length: int = 77
    vocab_size: int = 49408
    hf_tokenizer_name: Optional[str] = None
    tokenizer_kwargs: Optional[dict] = None
    width: int = 512
    heads: int = 8
    layers: int = 12
    mlp_ratio: float = 4.0
    ls_init_value: Optional[float] = None
    embed_cls: bool = False
    pad_id: int = 0
    no_causal_mask: bool = False
    final_ln_after_pool: bool = False
    pool_type: str = "argmax"
    proj_bias: bool = False
    proj_type: str = "linear"
    output_tokens: bool = False
    act_kwargs: Optional[dict] = None
    norm_kwargs: Optional[dict] = None
    hf_model_name: Optional[str] = None


def get_cast_dtype(precision: str):
    """reference model.py:87-93"""
    if precision == "bf16":
        return torch.bfloat16
    if precision == "fp16":
        return torch.float16
    return None


def get_input_dtype(precision: str):
    """reference model.py:96-102"""
    if precision in ("bf16", "pure_bf16"):
        return torch.bfloat16
    if precision in ("fp16", "pure_fp16"):
        return torch.float16
    return None


_PRECISION_NOTES = {
    "amp": "bf16 MFMA operands with fp32 accumulation, fp32 master weights and Adam moments, no loss scaling "
           "(the reference's `amp` is fp16 autocast + GradScaler; bf16 has fp32's exponent range, so no scaler is needed)",
    "amp_bf16": "bf16 MFMA operands with fp32 accumulation over fp32 master weights (what bf16 autocast computes)",
    "amp_bfloat16": "bf16 MFMA operands with fp32 accumulation over fp32 master weights (what bf16 autocast computes)",
    "bf16": "bf16 operands and activations, but fp32 master weights and Adam moments are KEPT (the reference's `bf16` "
            "casts Linear/Conv/attention weights to bf16 and lets AdamW keep bf16 moments)",
    "pure_bf16": "bf16 operands and activations, but fp32 master weights, LayerNorm parameters and Adam moments are KEPT "
                 "(the reference's `pure_bf16` casts every parameter)",
}
_PRECISION_NOTES["fp8"] = ("fp8 (OCP e4m3, one power-of-two scale per output channel) attention / MLP weights, bf16 activations, "
                          "fp32 accumulation, fp32 master weights and Adam moments; the dequantised weights are exact in bf16 and "
                          "feed the bf16 MFMA kernels (CDNA4 has no fp8 x bf16 MFMA); wgrad is bf16, straight-through to the masters")
_PRECISION_NOTES["fp8_mfma"] = ("fp8 (OCP e4m3) block weights AND forward activations (one power-of-two scale per weight row / "
                               "per activation row), multiplied on the CDNA4 fp8 MFMA (v_mfma_f32_16x16x128_f8f6f4: exact products, "
                               "fp32 sums) in every forward linear AND every dgrad of the residual blocks (gradient rows and the rows of "
                               "the transposed weight quantised the same way); wgrad is bf16 from the bf16 activations and gradients, "
                               "straight-through to the fp32 master weights; Adam moments fp32")
_PRECISION_TOLD = set()


def compute_dtype_for(precision: str) -> torch.dtype:
    """Kernel operand dtype for a `--precision` value: fp32 is the parity mode, the bf16 / amp modes run bf16 operands +
    fp32 accumulation (CDNA4 MFMA; fp16 has the same MFMA rate and a narrower range, so no fp16 path is built --
    fp16 / pure_fp16 are rejected rather than silently remapped)."""
    if precision in ("fp32", None):
        return torch.float32
    if precision in ("fp16", "pure_fp16"):
        raise NotImplementedError(
            f"--precision {precision}: this stack has no fp16 kernels (CDNA4 runs bf16 and fp16 MFMA at the same rate); "
            "use bf16 / amp_bf16 / amp, or fp32 for the parity mode")
    if precision not in _PRECISION_NOTES:
        raise ValueError(f"unknown precision {precision!r}")
    if precision not in _PRECISION_TOLD:
        _PRECISION_TOLD.add(precision)
        import logging
        logging.warning(f"colxlip_amd: --precision {precision} runs as: {_PRECISION_NOTES[precision]}")
    return torch.bfloat16


# --------------------------------------------------------------------------- parameter containers
class LayerNormParams(nn.Module):
    def __init__(self, width: int):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(width))
        self.bias = nn.Parameter(torch.zeros(width))


class LinearParams(nn.Module):
    def __init__(self, in_f: int, out_f: int, bias: bool = True):
        super().__init__()
        self.weight = nn.Parameter(torch.empty(out_f, in_f))
        self.bias = nn.Parameter(torch.empty(out_f)) if bias else None
        bound = 1.0 / math.sqrt(in_f)   # nn.Linear default (kaiming_uniform a=sqrt(5))
        nn.init.uniform_(self.weight, -bound, bound)
        if bias:
            nn.init.uniform_(self.bias, -bound, bound)


class ConvParams(nn.Module):
    """conv1 of the reference (transformer.py:549-555): weight [width, 3, P, P], no bias."""

    def __init__(self, width: int, patch: int):
        super().__init__()
        self.weight = nn.Parameter(torch.empty(width, 3, patch, patch))
        bound = 1.0 / math.sqrt(3 * patch * patch)
        nn.init.uniform_(self.weight, -bound, bound)


class AttentionParams(nn.Module):
    """nn.MultiheadAttention's packed parameters (transformer.py:228)."""

    def __init__(self, width: int):
        super().__init__()
        self.in_proj_weight = nn.Parameter(torch.empty(3 * width, width))
        self.in_proj_bias = nn.Parameter(torch.zeros(3 * width))
        self.out_proj = LinearParams(width, width)
        nn.init.xavier_uniform_(self.in_proj_weight)
        nn.init.zeros_(self.out_proj.bias)


class MlpParams(nn.Module):
    def __init__(self, width: int, mlp_width: int):
        super().__init__()
        self.c_fc = LinearParams(width, mlp_width)
        self.c_proj = LinearParams(mlp_width, width)


class ResidualAttentionBlock(nn.Module):
    """Parameter layout of transformer.py:213-240; compute lives in the tower engine."""

    def __init__(self, width: int, mlp_width: int):
        super().__init__()
        self.ln_1 = LayerNormParams(width)
        self.attn = AttentionParams(width)
        self.ln_2 = LayerNormParams(width)
        self.mlp = MlpParams(width, mlp_width)


class Transformer(nn.Module):
    def __init__(self, width: int, layers: int, heads: int, mlp_ratio: float = 4.0):
        super().__init__()
        self.width, self.layers, self.heads = width, layers, heads
        self.mlp_width = int(width * mlp_ratio)
        self.grad_checkpointing = False
        self.resblocks = nn.ModuleList([ResidualAttentionBlock(width, self.mlp_width) for _ in range(layers)])


# --------------------------------------------------------------------------- tower engine
_GEMM_SUFFIXES = ("attn.in_proj_weight", "attn.out_proj.weight", "mlp.c_fc.weight", "mlp.c_proj.weight")
_WGRAD_GROUP = os.environ.get("CLIPX_WGRAD_GROUP", "1") != "0"      # the four wgrads of a residual block as one launch (bf16)


_GELU8 = os.environ.get("CLIPX_GELU8", "1") != "0"
_POOLED_ATTN = os.environ.get("CLIPX_ATTN_POOLED", "1") != "0"     # 0: full attention + row gather in a pooled last block (A/B)


class _Engine:
    """Runs one tower (vision or text) forward/backward as a sequence of HIP kernel launches.

    `owner` is the nn.Module holding the parameters under the reference's names; `prefix` is ''
    for both (vision names are relative to `visual`, text names are top-level CLIP names)."""

    def __init__(self, kind: str, owner: nn.Module, tf: Transformer, seq: int, causal: bool, act: int,
                 embed_dim: int, names: List[str]):
        self.kind, self.owner, self.tf = kind, owner, tf
        self.seq, self.causal, self.act, self.embed_dim = seq, causal, act, embed_dim
        self.names = names                      # parameter names in Function-argument order
        self.width, self.heads, self.layers, self.mlp = tf.width, tf.heads, tf.layers, tf.mlp_width
        self.dtype = torch.float32
        self._shadow: Dict[str, Tuple[torch.Tensor, torch.Tensor, int, int]] = {}
        self._ws: Dict[str, torch.Tensor] = {}
        self._arena: Optional[torch.Tensor] = None
        self._arena_off: Dict[str, Tuple[int, int]] = {}
        self.P: Dict[str, torch.Tensor] = {}
        # data-parallel hand-over (distributed.GradSync.attach): begin(arena) before the first gradient kernel of a
        # backward, ready(flat fp32 view of finished gradients) per finished range, done(arena) after the last range
        self.grad_ready_hook = None
        self.grad_begin_hook = None
        self.grad_done_hook = None
        self.grad_late_hook = None              # (list of gradient tensors) when a backward could not use the arena ranges
        self.grad_start_hook = None             # (engine) at the start of EVERY backward, whichever way its gradients go
        self.peer = None                        # the model's other tower engine (shares the device's memory budget)
        self.grad_chunks = 4                    # early all-reduce ranges per backward (the arena's tail goes first)
        # Text tower: only positions 0..EOT of each caption are computed ("packed rows", ops.TextLayout) -- under the
        # causal mask + EOT pooling of the reference (transformer.py:839-855, 960-966) everything behind the EOT is dead.
        # CLIPX_TEXT_UNPAD=0 keeps the reference's dense [batch*77] layout.
        self.packed = kind == "text" and causal and os.environ.get("CLIPX_TEXT_UNPAD", "1") != "0"
        self._layout_key = None
        self._layout_cached = None
        self.last_layout = None
        # Last residual block: only the pooled token of each sample (CLS / EOT) is read from its output, so its out_proj, MLP
        # and their backward run on `batch` rows (exactly the same result; CLIPX_PRUNE_LAST=0 computes every token)
        self.prune_last = os.environ.get("CLIPX_PRUNE_LAST", "1") != "0"
        # ... and its in_proj as k | v on every row + q on the pooled rows (bf16 without weight / activation quantisation;
        # CLIPX_ATTN_POOLED_SPLIT=0: one GEMM over q | k | v)
        self.pooled_split = os.environ.get("CLIPX_ATTN_POOLED_SPLIT", "1") != "0"
        self.weight_quant = None                # "e4m3": the four GEMM weights of every block are fp8-quantised (precision fp8)
        self.act_quant = None                   # "e4m3": forward linears quantise their input rows and run on the fp8 MFMA

    # -- parameter access ---------------------------------------------------------------
    def bind(self, params: Dict[str, torch.Tensor]):
        self.P = params

    def _pw(self, name: str) -> torch.Tensor:
        """A parameter, or -- `<in_proj_weight>#q` / `#kv` -- the query rows / the key and value rows of a packed attention
        in_proj (nn.MultiheadAttention: rows [0, w) and [w, 3w)) as a view that shares the parameter's version counter."""
        if "#" in name:
            base, part = name.split("#")
            p = self.P[base].detach()
            w = p.shape[0] // 3
            return p[:w] if part == "q" else p[w:]
        return self.P[name]

    def _w2d(self, name: str) -> torch.Tensor:
        p = self._pw(name)
        return p.view(p.shape[0], -1) if p.ndim != 2 else p

    def W(self, name: str) -> torch.Tensor:
        """GEMM operand [N,K] in the compute dtype (fp32 master itself in parity mode)."""
        if self.dtype == torch.float32:
            return self._w2d(name)
        return self._refresh(name)[0]

    def Wt(self, name: str) -> Optional[torch.Tensor]:
        if self.dtype == torch.float32:
            return None
        return self._refresh(name)[1]

    def _refresh(self, name: str):
        p = self._pw(name)
        ent = self._shadow.get(name)
        if ent is None or ent[2] != p._version or ent[3] != p.data_ptr():
            w = self._w2d(name).detach()
            N, K = w.shape
            quant = self.weight_quant == "e4m3" and name.endswith(_GEMM_SUFFIXES)
            if ent is None or ent[0].device != w.device or (quant and len(ent) < 6):
                w16 = torch.empty((N, K), dtype=torch.bfloat16, device=w.device)
                wt16 = torch.empty((K, N), dtype=torch.bfloat16, device=w.device)
                w8 = torch.empty((N, K), dtype=torch.uint8, device=w.device) if quant else None
                rexp = torch.empty((N,), dtype=torch.int32, device=w.device) if quant else None
            else:
                w16, wt16 = ent[0], ent[1]
                w8, rexp = (ent[4], ent[5]) if quant else (None, None)
            if quant:
                ops.quant_weight_e4m3(w, rexp, w8, w16, wt16)
                ent = (w16, wt16, p._version, p.data_ptr(), w8, rexp)
                if self.act_quant == "e4m3" and N <= 8192 and N % 8 == 0:
                    # the dgrad operand: rows of the [K,N] copy, one exponent per input channel (e4m3 x 2^e values stay on the
                    # e4m3 grid under a second power-of-two scale unless they leave its exponent range)
                    wt8, wtexp = ops.quant_rows_e4m3(wt16)
                    ent = ent + (wt8, wtexp)
            else:
                ops.cast_weight(w, w16, wt16)
                ent = (w16, wt16, p._version, p.data_ptr())
            self._shadow[name] = ent
        return ent

    def _ln_fwd(self, x, gname: str, bname: str):
        """LayerNorm forward in front of a block linear: (y, mean, rstd, q8) with q8 = (e4m3 rows, exponents) when the consumer
        runs on the fp8 MFMA (precision fp8_mfma; quantised in the same pass), else None."""
        P = self.P
        w = x.shape[1]
        if self.act_quant == "e4m3" and x.dtype == torch.bfloat16 and w % 256 == 0 and 256 <= w <= 1280:
            y, mean, rstd, y8, ye = ops.layernorm_fwd_q8(x, P[gname], P[bname])
            return y, mean, rstd, (y8, ye)
        y, mean, rstd = ops.layernorm_fwd(x, P[gname], P[bname])
        return y, mean, rstd, None

    def _lin(self, x, wname: str, bias, act=None, want_preact=False, residual=None, q8=None):
        """Forward linear of a residual block.  Precision fp8_mfma: the input rows are quantised to e4m3 (one exponent per row)
        and multiplied with the e4m3 weight rows on the fp8 MFMA (K must be a multiple of 128, at least 256: every real model);
        otherwise the bf16 kernel on the (possibly dequantised) bf16 weight copy."""
        act = self.act if act is True else (ops.ACT_NONE if act is None else act)
        if want_preact and act == ops.ACT_GELU and x.dtype == torch.bfloat16 and residual is None and _GELU8:
            # the backward needs the pre-activation only for the factor GELU'(u): the epilogue keeps THAT, on eight bits
            # (csrc/gemm_epi.h G8_*; `u` is then a uint8 tensor that the dgrad wrappers recognise).  CLIPX_GELU8=0: bf16 u.
            want_preact = "gelu8"
        if self.act_quant == "e4m3" and x.dtype == torch.bfloat16 and x.shape[1] % 128 == 0 and 256 <= x.shape[1] <= 8192:
            ent = self._refresh(wname)
            if len(ent) >= 6 and ent[4] is not None:
                x8, xe = q8 if q8 is not None else ops.quant_rows_e4m3(x)
                return ops.linear_fwd_fp8(x8, xe, ent[4], ent[5], bias, act=act, want_preact=want_preact, residual=residual)
        return ops.linear_fwd(x, self.W(wname), bias, act=act, want_preact=want_preact, residual=residual)

    def _dgrad(self, dy, wname: str, act=None, u=None):
        """dx = dy @ W (optionally * act'(u)) of a residual block's linear.  Precision fp8_mfma: gradient rows quantised to e4m3
        and multiplied with the e4m3 rows of the transposed weight on the fp8 MFMA; otherwise the bf16 / fp32 kernels."""
        act = ops.ACT_NONE if act is None else act
        f32 = self.dtype == torch.float32
        if self.act_quant == "e4m3" and dy.dtype == torch.bfloat16 and dy.shape[1] % 128 == 0 and 256 <= dy.shape[1] <= 8192:
            ent = self._refresh(wname)
            if len(ent) >= 8:
                d8, de = ops.quant_rows_e4m3(dy)
                return ops.linear_dgrad_fp8(d8, de, ent[6], ent[7], act=act, u=u)
        return ops.linear_dgrad(dy, self.W(wname) if f32 else None, self.Wt(wname), act=act, u=u)

    def _refresh_all(self):
        """After an optimizer step every bf16 copy is stale: refresh them all in ONE launch (descriptor table built once,
        pointers are stable) instead of one launch per weight on first use."""
        if self.dtype == torch.float32 or len(self._shadow) < 2:
            return
        if self.weight_quant is not None:
            if os.environ.get("CLIPX_QUANT_MULTI", "1") != "0":         # 0: per-tensor quantisation on first use (A/B, tests)
                self._refresh_all_quant()
            return
        names = list(self._shadow.keys())
        ents = [self._shadow[n] for n in names]
        ps = [self._pw(n) for n in names]
        if not all(e[2] != p._version and e[3] == p.data_ptr() for e, p in zip(ents, ps)):
            return                                  # nothing (or only part) changed: the per-tensor path handles it
        key = tuple((p.data_ptr(), e[0].data_ptr(), e[1].data_ptr()) for e, p in zip(ents, ps))
        if getattr(self, "_cast_key", None) != key:
            import numpy as np
            rec = np.zeros(len(names), dtype=np.dtype([("w", "<u8"), ("w16", "<u8"), ("wt16", "<u8"), ("N", "<i4"), ("K", "<i4"),
                                                       ("block0", "<u4"), ("tiles_k", "<u4")]))
            blk = 0
            for i, (e, p) in enumerate(zip(ents, ps)):
                N, K = e[0].shape
                tk = (K + 31) // 32
                rec[i] = (p.data_ptr(), e[0].data_ptr(), e[1].data_ptr(), N, K, blk, tk)
                blk += ((N + 31) // 32) * tk
            assert rec.dtype.itemsize == 40
            self._cast_table = torch.from_numpy(rec.view(np.uint8).copy()).to(ents[0][0].device)
            self._cast_blocks = blk
            self._cast_key = key
        ops.cast_weight_multi(self._cast_table, len(names), self._cast_blocks)
        for n, e, p in zip(names, ents, ps):
            self._shadow[n] = (e[0], e[1], p._version, p.data_ptr())

    def _refresh_all_quant(self):
        """fp8 modes: re-quantise every block weight of the tower in three launches (clipx_quant_weight_multi) and refresh the
        plain bf16 copies of the other weights in one (clipx_cast_weight_multi); only when EVERY copy is stale at unchanged
        addresses (the state right after an optimizer step), else the per-tensor path handles what changed."""
        names = list(self._shadow.keys())
        ents = [self._shadow[n] for n in names]
        ps = [self.P[n] for n in names]
        if not all(e[2] != p._version and e[3] == p.data_ptr() for e, p in zip(ents, ps)):
            return
        import numpy as np
        qi = [i for i, e in enumerate(ents) if len(e) >= 6 and e[4] is not None]
        ci = [i for i, e in enumerate(ents) if not (len(e) >= 6 and e[4] is not None)]
        # every address the tables hold is part of the key: the per-tensor path allocates fresh e4m3 copies of the transposed
        # weight each time it runs, and a table built before that would write into freed memory
        key = tuple((ps[i].data_ptr(), len(ents[i])) + tuple(t.data_ptr() for t in ents[i][:2] + ents[i][4:] if t is not None)
                    for i in range(len(names)))
        if getattr(self, "_quant_key", None) != key:
            dev = ents[0][0].device
            rec = np.zeros(len(qi), dtype=np.dtype([("w", "<u8"), ("w8", "<u8"), ("w16", "<u8"), ("wt16", "<u8"), ("wt8", "<u8"),
                                                    ("rexp", "<u8"), ("wtexp", "<u8"), ("N", "<i4"), ("K", "<i4"), ("b0r", "<u4"),
                                                    ("b0t", "<u4"), ("b0x", "<u4"), ("tk", "<u4")]))
            br = bt = bx = 0
            for j, i in enumerate(qi):
                e, p = ents[i], ps[i]
                N, K = e[0].shape
                tk = (K + 31) // 32
                has_t = len(e) >= 8
                rec[j] = (p.data_ptr(), e[4].data_ptr(), e[0].data_ptr(), e[1].data_ptr(), e[6].data_ptr() if has_t else 0,
                          e[5].data_ptr(), e[7].data_ptr() if has_t else 0, N, K, br, bt, bx, tk)
                br += (N + 3) // 4
                bt += ((N + 31) // 32) * tk
                bx += (K + 3) // 4
            assert rec.dtype.itemsize == 80
            self._quant_table = torch.from_numpy(rec.view(np.uint8).copy()).to(dev) if qi else None
            self._quant_blocks = (br, bt, bx if any(len(ents[i]) >= 8 for i in qi) else 0)
            crec = np.zeros(len(ci), dtype=np.dtype([("w", "<u8"), ("w16", "<u8"), ("wt16", "<u8"), ("N", "<i4"), ("K", "<i4"),
                                                     ("block0", "<u4"), ("tiles_k", "<u4")]))
            blk = 0
            for j, i in enumerate(ci):
                e, p = ents[i], ps[i]
                N, K = e[0].shape
                tk = (K + 31) // 32
                crec[j] = (p.data_ptr(), e[0].data_ptr(), e[1].data_ptr(), N, K, blk, tk)
                blk += ((N + 31) // 32) * tk
            self._qcast_table = torch.from_numpy(crec.view(np.uint8).copy()).to(dev) if ci else None
            self._qcast_blocks = blk
            self._quant_key = key
        if qi:
            ops.quant_weight_multi(self._quant_table, len(qi), *self._quant_blocks)
        if ci:
            ops.cast_weight_multi(self._qcast_table, len(ci), self._qcast_blocks)
        for n, e, p in zip(names, ents, ps):
            self._shadow[n] = (e[0], e[1], p._version, p.data_ptr()) + tuple(e[4:])

    def _workspace(self, key: str, nbytes: int, device) -> torch.Tensor:
        t = self._ws.get(key)
        if t is None or t.numel() < nbytes or t.device != device:
            t = torch.empty((max(nbytes, 16),), dtype=torch.uint8, device=device)
            self._ws[key] = t
        return t

    # -- gradient targets -----------------------------------------------------------------
    def _new_arena(self, device):
        off = 0
        offs = {}
        for n in self.names:
            k = self.P[n].numel()
            offs[n] = (off, k)
            off += (k + 3) // 4 * 4
        return torch.zeros((off,), dtype=torch.float32, device=device), offs     # pads between slots stay zero

    def _in_arena(self, g: torch.Tensor) -> bool:
        a = self._arena
        return (g.dtype == torch.float32 and g.is_contiguous() and g.device == a.device
                and a.data_ptr() <= g.data_ptr() < a.data_ptr() + 4 * a.numel())

    def _begin_grads(self, device):
        if self.grad_start_hook is not None:
            self.grad_start_hook(self)
        if self._arena is None or self._arena.device != device:
            self._arena, self._arena_off = self._new_arena(device)
        # Re-entrancy: if this tower ran twice inside one autograd graph, the first node's gradient views are still
        # sitting in autograd's input buffers (not yet installed as .grad) when the second node's backward starts.
        # Writing the persistent arena again (beta = 0) would alias them.  Detect it -- more tensors share the arena's
        # storage than there are installed .grad views -- and give THIS backward a private arena.
        installed = sum(1 for n in self.names if self.P[n].grad is not None and self._in_arena(self.P[n].grad))
        try:
            holders = torch._C._storage_Use_Count(self._arena.untyped_storage()._cdata) - 2   # the arena + this wrapper
        except AttributeError:      # private symbol gone: assume the worst only when a second backward of this tower is pending
            holders = installed + (1 if getattr(self, "_open_backwards", 0) > 1 else 0)
        clash = holders > installed
        if clash:
            if not getattr(self, "_clash_told", False):
                self._clash_told = True
                import logging
                logging.warning(f"colxlip_amd: {self.kind} tower: {holders} tensors share the gradient arena but only {installed} are "
                                "installed .grad views (the tower ran twice in one graph, or something else holds a gradient view): "
                                "this backward writes a private arena and its gradients are reduced late, not overlapped")
            self._cur, self._cur_off = self._new_arena(device)
        else:
            self._cur, self._cur_off = self._arena, self._arena_off
        self._gout: Dict[str, Optional[torch.Tensor]] = {}
        self._gbeta: Dict[str, float] = {}
        # Early hand-over to the data-parallel synchroniser, a range at a time: only when every gradient of this
        # backward lives in the persistent arena -- fresh views (beta = 0) or accumulation into views installed by an
        # earlier backward (beta = 1, gradient accumulation) -- see _grads_ready().
        self._early_ok = (self.grad_ready_hook is not None and not clash and
                          all(self.P[n].grad is None or self._in_arena(self.P[n].grad) for n in self.names))
        self._hi_done = self._cur.numel()
        self._by_off = sorted(self.names, key=lambda n: self._cur_off[n][0])
        if self._early_ok and self.grad_begin_hook is not None:
            self.grad_begin_hook(self._arena)       # later writers wait for in-flight reductions of this arena

    def _grads_ready(self, done_from_block: int):
        """Blocks >= done_from_block and the head (final LayerNorm, projection) have all their gradient kernels
        enqueued: hand the largest finished TAIL of the arena to the synchroniser (the arena is laid out in parameter
        order, so the tail is the last blocks; whatever ordering `names` has, a range is only released when every
        tensor in it is finished)."""
        if not self._early_ok:
            return
        head = ("ln_post.", "ln_final.", "proj", "text_projection")
        def finished(n: str) -> bool:
            if n.startswith("transformer.resblocks."):
                return int(n.split(".")[2]) >= done_from_block
            return n.startswith(head) and not n.startswith("proj.")
        lo = self._hi_done
        for n in reversed(self._by_off):
            off, _ = self._cur_off[n]
            if off >= self._hi_done:
                continue
            if not finished(n):
                break
            lo = off
        if lo < self._hi_done:
            self.grad_ready_hook(self._cur[lo:self._hi_done])
            self._hi_done = lo

    def G(self, name: str) -> Tuple[torch.Tensor, float]:
        """(fp32 buffer to write the gradient of `name` into, beta).  A parameter whose .grad is
        None gets a fresh arena view that the Function returns (autograd installs it, beta=0);
        an existing .grad is accumulated into in place (beta=1) and None is returned."""
        if name in self._gbeta:
            g = self._gout[name] if self._gout[name] is not None else self.P[name].grad
            return g, 1.0
        p = self.P[name]
        if p.grad is not None and p.grad.dtype == torch.float32 and p.grad.is_contiguous():
            self._gout[name] = None
            self._gbeta[name] = 1.0
            return p.grad, 1.0
        off, k = self._cur_off[name]
        g = self._cur[off:off + k].view(p.shape)
        self._gout[name] = g
        self._gbeta[name] = 0.0
        return g, 0.0

    def _finish_grads(self) -> List[Optional[torch.Tensor]]:
        # hand over the only references: autograd installs a returned gradient as .grad without a deep copy
        # only if nothing else refers to it, and GradSync / the optimizer want .grad to stay an arena view.
        out = [self._gout.get(n) for n in self.names]
        self._gout = {}
        self._gbeta = {}
        if self._early_ok:
            # every gradient of this tower now sits in the flat arena: let the data-parallel synchroniser start the
            # all-reduce of what _grads_ready() has not released yet while the other tower's backward is still running
            if self._hi_done > 0:
                self.grad_ready_hook(self._arena[:self._hi_done])
                self._hi_done = 0
            if self.grad_done_hook is not None:
                self.grad_done_hook(self._arena)
        elif self.grad_ready_hook is not None and self.grad_late_hook is not None:
            # gradients of this backward are not (all) in the persistent arena -- private arena of a re-entrant call, or a
            # foreign .grad being accumulated into: hand the tensors over one by one
            self.grad_late_hook([g if g is not None else self.P[n].grad for n, g in zip(self.names, out)])
        self._cur = None
        return out

    # -- one residual block -----------------------------------------------------------------
    def _block_fwd(self, x, i: int, batch: int, L: int, layout=None, need_out: bool = True):
        P, pre = self.P, f"transformer.resblocks.{i}."
        a, mean1, rstd1, a8 = self._ln_fwd(x, pre + "ln_1.weight", pre + "ln_1.bias")
        qkv = self._lin(a, pre + "attn.in_proj_weight", P[pre + "attn.in_proj_bias"], q8=a8)
        if layout is not None:
            o = ops.attention_packed_fwd(qkv, layout, self.heads, self.causal)
        else:
            # (the online-softmax kernels hand their log-sum-exp to the backward: it rides on the saved output tensor)
            o, lse = ops.attention_fwd(qkv, batch, L, self.heads, self.causal, want_lse=True)
            o.clipx_lse = lse
        x1 = self._lin(o, pre + "attn.out_proj.weight", P[pre + "attn.out_proj.bias"], residual=x)
        c, mean2, rstd2, c8 = self._ln_fwd(x1, pre + "ln_2.weight", pre + "ln_2.bias")
        h, u = self._lin(c, pre + "mlp.c_fc.weight", P[pre + "mlp.c_fc.bias"], act=True, want_preact=True, q8=c8)
        # need_out=False: the recompute of a checkpointed block in the backward -- everything the block's backward reads has been
        # produced by now; the block's OUTPUT (the c_proj GEMM, a third of the block's forward GEMM work) is not among it
        x2 = self._lin(h, pre + "mlp.c_proj.weight", P[pre + "mlp.c_proj.bias"], residual=x1) if need_out else None
        return x2, (x, a, mean1, rstd1, qkv, o, x1, c, mean2, rstd2, u, h)

    def _ln_finish(self, ws, width, gname, bname, colsum_name):
        outs = [None, None, None]
        betas = []
        for which, name in ((0, gname), (1, bname), (2, colsum_name)):
            if name is not None:
                outs[which], beta = self.G(name)
                betas.append(beta)
        if not betas:
            return
        if all(b == betas[0] for b in betas):          # the usual case: one launch for the three reductions
            ops.layernorm_bwd_finish(width, ws, outs[0], outs[1], outs[2], betas[0])
            return
        k = 0
        for which in range(3):
            if outs[which] is not None:
                args = [None, None, None]
                args[which] = outs[which]
                ops.layernorm_bwd_finish(width, ws, args[0], args[1], args[2], betas[k])
                k += 1

    def _block_bwd(self, dx2, saved, i: int, batch: int, L: int, prev_bias: Optional[str], layout=None):
        """dx2: grad of the block output.  The bias grad of this block's c_proj (= colsum(dx2)) was
        already produced by whoever made dx2.  Returns grad of the block input; colsum of it is
        folded into `prev_bias` (previous block's c_proj.bias) when given."""
        P, pre = self.P, f"transformer.resblocks.{i}."
        x, a, mean1, rstd1, qkv, o, x1, c, mean2, rstd2, u, h = saved
        M = dx2.shape[0]
        dev = dx2.device
        ws_ln = self._workspace("ln", ops.layernorm_ws_bytes(self.width), dev)
        f32 = self.dtype == torch.float32
        # The four wgrads of the block reduce over the same M rows: in bf16 they are launched as ONE grid at the end of the
        # block's backward (ops.linear_wgrad_group: 108 output tiles for a ViT-B/32 vision block instead of 36 / 36 / 9 / 27,
        # row split 2 ways instead of 7-28, a fifth of the fp32 slab traffic).  For that dx2 and dx1 must survive until then, so
        # the LayerNorm backwards write their outputs to fresh buffers instead of over their residual-gradient input (same bytes
        # moved).  CLIPX_WGRAD_GROUP=0 / fp32: one launch per wgrad, at the point its operands are ready, as before.
        grouped = (not f32) and _WGRAD_GROUP
        shapes = [(self.width, self.mlp), (self.mlp, self.width), (self.width, self.width), (3 * self.width, self.width)]
        if grouped:
            wsb = ops.linear_wgrad_group_ws_bytes(self.dtype, M, shapes)
        else:
            wsb = max(ops.linear_wgrad_ws_bytes(self.dtype, M, n_, k_) for n_, k_ in shapes)
        ws_wg = self._workspace("wgrad", wsb, dev)
        pending = []

        def wgrad(dy, xin, wname, bname=None):
            g, beta = self.G(wname)
            gb, beta_b = self.G(bname) if bname is not None else (None, 0.0)
            if grouped:
                pending.append((dy, xin, g, beta, gb, beta_b))
            else:
                ops.linear_wgrad(dy, xin, g, beta, ws_wg, db=gb, beta_b=beta_b)

        # MLP: GELU' rides in the c_proj dgrad epilogue, the c_fc bias gradient in the c_fc wgrad pass
        wgrad(dx2, h, pre + "mlp.c_proj.weight")
        du = self._dgrad(dx2, pre + "mlp.c_proj.weight", act=self.act, u=u)
        wgrad(du, c, pre + "mlp.c_fc.weight", pre + "mlp.c_fc.bias")
        dc = self._dgrad(du, pre + "mlp.c_fc.weight")
        dx1 = ops.layernorm_bwd(dc, x1, P[pre + "ln_2.weight"], mean2, rstd2, ws_ln, dx_res=dx2,
                                dx_out=None if grouped else dx2)          # not grouped: in place over dx2
        self._ln_finish(ws_ln, self.width, pre + "ln_2.weight", pre + "ln_2.bias", pre + "attn.out_proj.bias")
        # attention
        wgrad(dx1, o, pre + "attn.out_proj.weight")
        do = self._dgrad(dx1, pre + "attn.out_proj.weight")
        if layout is not None:
            dqkv = ops.attention_packed_bwd(qkv, do, layout, self.heads, self.causal)
        else:
            dqkv = ops.attention_bwd(qkv, do, batch, L, self.heads, self.causal, out=o, lse=getattr(o, "clipx_lse", None))
        wgrad(dqkv, a, pre + "attn.in_proj_weight", pre + "attn.in_proj_bias")
        da = self._dgrad(dqkv, pre + "attn.in_proj_weight")
        dx0 = ops.layernorm_bwd(da, x, P[pre + "ln_1.weight"], mean1, rstd1, ws_ln, dx_res=dx1,
                                dx_out=None if grouped else dx1)          # not grouped: in place over dx1
        self._ln_finish(ws_ln, self.width, pre + "ln_1.weight", pre + "ln_1.bias", prev_bias)
        if pending:
            ops.linear_wgrad_group(pending, ws_wg)
        return dx0

    # -- the last block when only the pooled rows of its output are consumed -------------------------------------------
    def _block_fwd_pooled(self, x, i: int, batch: int, L: int, layout, idx):
        """Attention as usual (every key/value is needed), then out_proj + residual, LayerNorm and the MLP on the `batch`
        pooled rows only.  Returns (x2 of the pooled rows [batch, width], saved)."""
        P, pre = self.P, f"transformer.resblocks.{i}."
        a, mean1, rstd1, a8 = self._ln_fwd(x, pre + "ln_1.weight", pre + "ln_1.bias")
        max_len = layout.longest if layout is not None else L
        pooled_ok = _POOLED_ATTN and ops.attention_pooled_supported(a.dtype, max_len, self.width // self.heads)
        if pooled_ok and self.pooled_split and self.weight_quant is None and self.act_quant is None:
            # Nobody reads the queries of the other rows either: the in_proj runs as k | v on every row and q on the pooled rows
            # (a third of this linear's forward, dgrad and wgrad saved; `#q` / `#kv`: row ranges of the packed in_proj weight)
            wn, w = pre + "attn.in_proj_weight", self.width
            bias = P[pre + "attn.in_proj_bias"].detach()
            a_s = ops.gather_rows(a, idx)
            kv = ops.linear_fwd(a, self.W(wn + "#kv"), bias[w:])
            q_s = ops.linear_fwd(a_s, self.W(wn + "#q"), bias[:w])
            o_s, lse = ops.attention_pooled_fwd_split(q_s, kv, idx, batch, L, self.heads, self.causal, layout)
            o_s.clipx_pooled_lse = lse
            qkv = (q_s, kv, a_s)
        else:
            qkv = self._lin(a, pre + "attn.in_proj_weight", P[pre + "attn.in_proj_bias"], q8=a8)
        if isinstance(qkv, tuple):
            pass
        elif pooled_ok:
            # one query row per sequence: O(L d) instead of the whole L x L attention (the log-sum-exp rides on the output)
            o_s, lse = ops.attention_pooled_fwd(qkv, idx, batch, L, self.heads, self.causal, layout)
            o_s.clipx_pooled_lse = lse
        else:
            if layout is not None:
                o = ops.attention_packed_fwd(qkv, layout, self.heads, self.causal)
            else:
                o = ops.attention_fwd(qkv, batch, L, self.heads, self.causal)
            o_s = ops.gather_rows(o, idx)
        x_s = ops.gather_rows(x, idx)
        x1 = self._lin(o_s, pre + "attn.out_proj.weight", P[pre + "attn.out_proj.bias"], residual=x_s)
        c, mean2, rstd2, c8 = self._ln_fwd(x1, pre + "ln_2.weight", pre + "ln_2.bias")
        h, u = self._lin(c, pre + "mlp.c_fc.weight", P[pre + "mlp.c_fc.bias"], act=True, want_preact=True, q8=c8)
        x2 = self._lin(h, pre + "mlp.c_proj.weight", P[pre + "mlp.c_proj.bias"], residual=x1)
        return x2, (x, a, mean1, rstd1, qkv, o_s, x1, c, mean2, rstd2, u, h)

    def _block_bwd_pooled(self, dx2, saved, i: int, batch: int, L: int, prev_bias: Optional[str], layout, idx):
        """Backward of _block_fwd_pooled.  dx2 [batch, width]: gradient of the pooled rows of the block output (the rest of
        that gradient is exactly zero).  Returns the dense gradient of the block input."""
        P, pre = self.P, f"transformer.resblocks.{i}."
        x, a, mean1, rstd1, qkv, o_s, x1, c, mean2, rstd2, u, h = saved
        M, b = x.shape[0], dx2.shape[0]
        dev = dx2.device
        f32 = self.dtype == torch.float32
        ws_ln = self._workspace("ln", ops.layernorm_ws_bytes(self.width), dev)
        wsb = max(ops.linear_wgrad_ws_bytes(self.dtype, M, 3 * self.width, self.width),
                  ops.linear_wgrad_ws_bytes(self.dtype, b, self.mlp, self.width),
                  ops.linear_wgrad_ws_bytes(self.dtype, b, self.width, self.mlp),
                  ops.colsum_ws_bytes(b, self.width))
        ws_wg = self._workspace("wgrad", wsb, dev)

        def W(n):
            return self.W(pre + n) if f32 else None

        g, beta = self.G(pre + "mlp.c_proj.weight")
        ops.linear_wgrad(dx2, h, g, beta, ws_wg)
        du = ops.linear_dgrad(dx2, W("mlp.c_proj.weight"), self.Wt(pre + "mlp.c_proj.weight"), act=self.act, u=u)
        g, beta = self.G(pre + "mlp.c_fc.weight")
        gb, beta_b = self.G(pre + "mlp.c_fc.bias")
        ops.linear_wgrad(du, c, g, beta, ws_wg, db=gb, beta_b=beta_b)
        dc = ops.linear_dgrad(du, W("mlp.c_fc.weight"), self.Wt(pre + "mlp.c_fc.weight"))
        dx1 = ops.layernorm_bwd(dc, x1, P[pre + "ln_2.weight"], mean2, rstd2, ws_ln, dx_res=dx2, dx_out=dx2)   # in place
        self._ln_finish(ws_ln, self.width, pre + "ln_2.weight", pre + "ln_2.bias", pre + "attn.out_proj.bias")
        g, beta = self.G(pre + "attn.out_proj.weight")
        ops.linear_wgrad(dx1, o_s, g, beta, ws_wg)
        do_s = ops.linear_dgrad(dx1, W("attn.out_proj.weight"), self.Wt(pre + "attn.out_proj.weight"))
        lse = getattr(o_s, "clipx_pooled_lse", None)
        if isinstance(qkv, tuple):
            q_s, kv, a_s = qkv
            w, wn = self.width, pre + "attn.in_proj_weight"
            dq_s, dkv = ops.attention_pooled_bwd_split(q_s, kv, do_s, lse, idx, batch, L, self.heads, self.causal, layout)
            g, beta = self.G(wn)
            gb, beta_b = self.G(pre + "attn.in_proj_bias")
            ops.linear_wgrad(dkv, a, g[w:], beta, ws_wg, db=gb[w:], beta_b=beta_b)
            ops.linear_wgrad(dq_s, a_s, g[:w], beta, ws_wg, db=gb[:w], beta_b=beta_b)
            da = ops.linear_dgrad(dkv, None, self.Wt(wn + "#kv"))
            ops.scatter_add_rows(ops.linear_dgrad(dq_s, None, self.Wt(wn + "#q")), idx, da)
            dx0 = ops.layernorm_bwd(da, x, P[pre + "ln_1.weight"], mean1, rstd1, ws_ln)
            self._ln_finish(ws_ln, self.width, pre + "ln_1.weight", pre + "ln_1.bias", prev_bias)
            ops.scatter_add_rows(dx1, idx, dx0)
            if prev_bias is not None:
                gp, _ = self.G(prev_bias)
                ops.colsum(dx1, gp, 1.0, ws_wg)
            return dx0
        if lse is not None:
            dqkv = ops.attention_pooled_bwd(qkv, do_s, lse, idx, batch, L, self.heads, self.causal, layout)
        else:
            do = ops.scatter_rows(do_s, idx, M)                    # zero except the pooled query rows
            if layout is not None:
                dqkv = ops.attention_packed_bwd(qkv, do, layout, self.heads, self.causal)
            else:
                dqkv = ops.attention_bwd(qkv, do, batch, L, self.heads, self.causal)
            del do
        g, beta = self.G(pre + "attn.in_proj_weight")
        gb, beta_b = self.G(pre + "attn.in_proj_bias")
        ops.linear_wgrad(dqkv, a, g, beta, ws_wg, db=gb, beta_b=beta_b)
        da = ops.linear_dgrad(dqkv, W("attn.in_proj_weight"), self.Wt(pre + "attn.in_proj_weight"))
        dx0 = ops.layernorm_bwd(da, x, P[pre + "ln_1.weight"], mean1, rstd1, ws_ln)
        self._ln_finish(ws_ln, self.width, pre + "ln_1.weight", pre + "ln_1.bias", prev_bias)
        ops.scatter_add_rows(dx1, idx, dx0)                    # the residual path carries dx1 on the pooled rows only
        if prev_bias is not None:                              # ... and so does the previous c_proj's bias gradient
            gp, _ = self.G(prev_bias)
            ops.colsum(dx1, gp, 1.0, ws_wg)
        return dx0

    # -- projection `pooled @ proj` with proj stored [width, embed] ---------------------------
    def _proj_fwd(self, pooled, name: str):
        b = pooled.shape[0]
        if self.dtype == torch.float32:
            proj = self.P[name]
            y = torch.empty((b, self.embed_dim), dtype=torch.float32, device=pooled.device)
            ops.gemm_f32(b, self.embed_dim, self.width, pooled, self.width, 1, proj, self.embed_dim, 1, y,
                         self.embed_dim)
            return y
        return ops.linear_fwd(pooled, self.Wt(name), out_dtype=torch.float32)     # Wt = proj^T [E, width]

    # -- whole-tower forward / backward ---------------------------------------------------------
    def forward(self, inp: torch.Tensor, save: bool, want_tokens: bool = False):
        """want_tokens (ColXLIP, reference model.py:529-575): also return the final LayerNorm applied to EVERY token,
        as a [M + 1, width] buffer whose extra last row is zero (the row masked text positions are read from)."""
        P = self.P
        self._refresh_all()
        ckpt = self.tf.grad_checkpointing and save
        L = self.seq
        if self.kind == "vision":
            batch = inp.shape[0]
            owner = self.owner
            # patch dropout (reference transformer.py:712): while training, only the kept patches are embedded and every block
            # runs on 1 + keep rows per image; the mask and L travel in ctx to the backward and the checkpoint recompute
            pd = owner.patch_dropout
            keep_idx = pd.draw(batch, self.seq - 1, inp.device) if (owner.training and pd.prob > 0) else None
            if keep_idx is None:
                patches = ops.patchify(inp, owner.patch_size[0], owner.k_padded(self.dtype), self.dtype)
                tok = ops.linear_fwd(patches, self._conv_w(), None)
                x0 = ops.vision_assemble(tok, P["class_embedding"], P["positional_embedding"], batch, self.seq)
            else:
                L = 1 + keep_idx.shape[1]
                patches = ops.patchify_keep(inp, owner.patch_size[0], owner.k_padded(self.dtype), self.dtype, keep_idx)
                tok = ops.linear_fwd(patches, self._conv_w(), None)
                x0 = ops.vision_assemble_keep(tok, P["class_embedding"], P["positional_embedding"], keep_idx, self.seq - 1)
            x, mean0, rstd0 = ops.layernorm_fwd(x0, P["ln_pre.weight"], P["ln_pre.bias"])
            head = (patches, x0, mean0, rstd0, keep_idx)
        else:
            batch = inp.shape[0]
            hd = self.width // self.heads          # packed attention kernels: head dim 64 (bf16), 32 / 64 / 80 (fp32)
            can_pack = (hd == 64 and (self.seq <= 128 or self.dtype == torch.float32)) or (self.dtype == torch.float32 and hd in (32, 80))
            layout = self._text_layout(inp) if (self.packed and can_pack and inp.shape[0] <= 8192) else None
            if layout is not None:
                x = ops.text_embed_packed(layout, P["token_embedding.weight"], P["positional_embedding"], self.dtype)
            else:
                x = ops.text_embed(inp, P["token_embedding.weight"], P["positional_embedding"], self.dtype)
            head = (inp, layout)
        layout = head[1] if self.kind == "text" else None
        self.last_layout = layout
        if self.kind == "vision":
            idx = ops.stride_index(batch, L, x.device)
        else:
            idx = layout.eot_rows if layout is not None else ops.eot_index(inp)
        pruned = self.prune_last and not want_tokens and self.layers > 0
        x_first = x
        for attempt in (0, 1):
            blocks = []
            x = x_first
            keep = self._ckpt_keep(x) if ckpt else self.layers      # blocks (the last ones) whose activations are kept whole
            try:
                for i in range(self.layers):
                    x_in = x
                    if pruned and i == self.layers - 1:
                        x, sv = self._block_fwd_pooled(x, i, batch, L, layout, idx)
                    else:
                        x, sv = self._block_fwd(x, i, batch, L, layout)
                    if save:
                        blocks.append(sv if i >= self.layers - keep else (x_in,))
                break
            except torch.cuda.OutOfMemoryError:
                # the split was sized from an estimate; when it was too generous, fall back to the reference's every-block
                # recompute and run the blocks again (nothing of this forward has been handed to autograd yet)
                if attempt == 1 or not ckpt or os.environ.get("CLIPX_CKPT_KEEP", "") != "":
                    raise
                blocks = sv = x = x_in = None
                if not self._ckpt_oom():
                    raise
        ln = "ln_post" if self.kind == "vision" else "ln_final"
        if pruned:      # x already holds the pooled rows only
            pooled, meanp, rstdp = ops.layernorm_fwd(x, P[ln + ".weight"], P[ln + ".bias"])
        else:
            pooled, meanp, rstdp = ops.layernorm_fwd(x, P[ln + ".weight"], P[ln + ".bias"], rows=batch, row_index=idx)
        feat = self._proj_fwd(pooled, "proj" if self.kind == "vision" else "text_projection")
        tok_all = mean_all = rstd_all = None
        if want_tokens:
            ln = "ln_post" if self.kind == "vision" else "ln_final"
            M = x.shape[0]
            tok_all = torch.empty((M + 1, self.width), dtype=x.dtype, device=x.device)
            tok_all[M].zero_()
            _, mean_all, rstd_all = ops.layernorm_fwd(x, P[ln + ".weight"], P[ln + ".bias"], out=tok_all[:M])
        ctx = (batch, head, blocks, x, idx, pooled, meanp, rstdp, ckpt, mean_all, rstd_all, pruned, L) if save else None
        if want_tokens:
            return feat, ctx, tok_all
        return feat, ctx

    def _state_bytes_to_come(self) -> int:
        """Bytes this tower will still allocate AFTER the forward that sizes the checkpoint split, from what exists now: the fp32
        gradient arena (4 B / parameter) and, with it, the two Adam moments the optimizer creates at its first step (8 B) while
        no backward has run; the bf16 operand copies W and W^T of the matrices (2 x 2 B) while they have not been made.  The
        first forward of a run sees none of them -- sizing the kept activations from the free memory alone handed out what the
        first backward and optimizer step then needed (advisor finding, round 3)."""
        if self.P:
            n = sum(p.numel() for p in self.P.values())
        else:                                  # parameters are bound at the first forward
            owned = dict(self.owner.named_parameters())
            n = sum(owned[k].numel() for k in self.names if k in owned)
        need = 0
        if self._arena is None:
            need += 12 * n
        if self.dtype != torch.float32 and len(self._shadow) < 2:
            need += 4 * n
        return need

    def _ckpt_keep(self, x: torch.Tensor) -> int:
        """Gradient checkpointing (reference transformer.py:499-504: every block recomputed) spends a forward to save memory; the
        MI355X has 288 GB of it.  So recompute only what does not fit: the LAST `keep` blocks store their activations as without
        checkpointing, the others only their input.  Same gradients bit for bit whatever `keep` is.  A block's activations are
        (7 + 2 mlp/width) x its input (a, qkv, o, x1, c, u, h; 1.5 mlp/width with the 8-bit GELU'); the budget is 82 % (8 % for the
        text tower) of what the allocator can still hand out when the step's first forward starts LESS the training state that
        does not exist yet (both towers' `_state_bytes_to_come`), less every block's input.  A tower whose whole need is under 5 % keeps everything.  CLIPX_CKPT_KEEP=n fixes
        the count (0 = the reference's behaviour).  Decided once per input shape, only by forwards that save for a backward
        (`ckpt` is false under no_grad); an out-of-memory error in a forward or backward drops the count to 0 (`_ckpt_oom`).
        `mem_get_info` is device-wide: ranks SHARING one device (a test rehearsal, not a deployment) each see the other's
        memory as free and should pin CLIPX_CKPT_KEEP."""
        env = os.environ.get("CLIPX_CKPT_KEEP", "")
        if env != "":
            return max(0, min(self.layers, int(env)))
        if not x.is_cuda:
            return 0
        key = (tuple(x.shape), x.dtype)
        cached = getattr(self, "_keep_cache", None)
        if cached is not None and cached[0] == key:
            return cached[1]
        unit = x.numel() * x.element_size()
        per_block = (7.0 + (1.5 if (_GELU8 and self.act == ops.ACT_GELU and x.dtype == torch.bfloat16) else 2.0) * self.mlp / self.width) * unit
        free, _total = torch.cuda.mem_get_info(x.device)
        avail = free + torch.cuda.memory_reserved(x.device) - torch.cuda.memory_allocated(x.device)
        to_come = self._state_bytes_to_come() + (self.peer._state_bytes_to_come() if getattr(self, "peer", None) is not None else 0)
        avail = max(0, avail - to_come)
        if per_block * self.layers <= 0.05 * avail:
            keep = self.layers
        else:
            # The step's peak is the END OF THE FORWARD -- every block's input + the kept blocks' activations -- once two or more
            # blocks are kept: the backward frees the kept (last) blocks first, and what they held is more than a recomputed
            # block's working set (measured, ViT-L/14-336 b = 1024: peak 30 + 15.5 keep GiB = "after forward" + 0.7 for keep = 8 ..
            # 14, profiles/r04_ckpt_keep_sweep.txt; the `+ 30 inputs` of round 3 counted that working set on top).  82 % of what is
            # available for the vision tower (8 % for the text tower, the rest for the allocator's slack -- 16 GiB reserved beyond
            # allocated at 214 GiB -- and for `per_block` being ~6 % short of the measured 15.5 GiB): 12 of 24 blocks there instead
            # of 10 (8 before the 8-bit GELU'), 1355 instead of 1384 (1408) ms/step.  At 85 % ViT-H/14 b = 2048 ran with 97 % of the
            # HBM reserved: too close.
            share = 0.82 if self.kind == "vision" else 0.08
            keep = int(max(0, min(self.layers, (share * avail - self.layers * unit) // per_block)))
            if keep < 2:          # nothing (or too little) is freed before the first recompute: its working set must fit beside the inputs
                keep = int(max(0, min(self.layers, (share * avail - (self.layers + 30) * unit) // per_block)))
        self._keep_cache = (key, keep)
        import logging
        logging.info(f"colxlip_amd: {self.kind} tower, gradient checkpointing: {keep} of {self.layers} blocks keep their activations "
                     f"({per_block / 2**30:.1f} GiB each, {avail / 2**30:.0f} GiB available after {to_come / 2**30:.1f} GiB of training "
                     f"state still to be allocated), {self.layers - keep} are recomputed")
        return keep

    def _ckpt_oom(self) -> bool:
        """An allocation failed while this tower kept activations under gradient checkpointing: keep none from now on (the
        reference's behaviour) and give the cached blocks back.  True when that changes anything, i.e. a retry can help."""
        cached = getattr(self, "_keep_cache", None)
        if cached is None:
            return False
        had = cached[1]
        self._keep_cache = (cached[0], 0)
        torch.cuda.empty_cache()
        import logging
        logging.warning(f"colxlip_amd: {self.kind} tower ran out of memory with {had} blocks' activations kept under "
                        "--grad-checkpointing: every block is recomputed from now on")
        return bool(had)

    def _text_layout(self, text: torch.Tensor):
        """Packed row layout of this batch of captions.  Building it costs one tiny kernel and an 8-integer read-back
        (a stream sync).  Only the SAME tensor object at the same version reuses a layout (an eval loop re-encoding one
        batch, a benchmark replaying one batch): the cache keeps that tensor alive, so a new batch can never be mistaken for
        it through a recycled device address."""
        hit = (self._layout_cached is not None and self._layout_key is not None and self._layout_key[0] is text
               and self._layout_key[1] == text._version)
        if not hit:
            self._layout_cached = ops.TextLayout(text, self.P["token_embedding.weight"].shape[0])
            self._layout_key = (text, text._version)
        return self._layout_cached

    def _conv_w(self):
        if self.dtype == torch.float32:
            return self._w2d("conv1.weight")
        return self.owner.conv_shadow(self)

    def backward(self, ctx, dfeat: Optional[torch.Tensor], dtok_all: Optional[torch.Tensor] = None) -> List[Optional[torch.Tensor]]:
        try:
            return self._backward(ctx, dfeat, dtok_all)
        except torch.cuda.OutOfMemoryError as e:
            # not retried here: part of this backward's gradients may already be accumulated.  The following steps recompute
            # every block; this one is the caller's to repeat (zero_grad + forward + backward).
            if ctx[8] and os.environ.get("CLIPX_CKPT_KEEP", "") == "" and self._ckpt_oom():
                raise torch.cuda.OutOfMemoryError(str(e) + "  [colxlip_amd: this backward kept activations under --grad-checkpointing; "
                                                  "the split has been reset to recompute every block -- repeat the step]") from e
            raise

    def _backward(self, ctx, dfeat: Optional[torch.Tensor], dtok_all: Optional[torch.Tensor] = None) -> List[Optional[torch.Tensor]]:
        P = self.P
        batch, head, blocks, x_last, idx, pooled, meanp, rstdp, ckpt, mean_all, rstd_all, pruned, L = ctx
        if dfeat is None:
            dfeat = torch.zeros((batch, self.embed_dim), dtype=torch.float32, device=x_last.device)
        dev = dfeat.device
        self._begin_grads(dev)
        M = x_last.shape[0]
        ws_ln = self._workspace("ln", ops.layernorm_ws_bytes(self.width), dev)
        proj_name = "proj" if self.kind == "vision" else "text_projection"
        ln_name = "ln_post" if self.kind == "vision" else "ln_final"
        dfeat = dfeat.contiguous()
        if dfeat.dtype != torch.float32:
            dfeat = dfeat.float()
        # projection
        g, beta = self.G(proj_name)
        if self.dtype == torch.float32:
            proj = P[proj_name]
            dpooled = torch.empty_like(pooled)
            ops.gemm_f32(batch, self.width, self.embed_dim, dfeat, self.embed_dim, 1, proj, 1, self.embed_dim,
                         dpooled, self.width)
            ops.gemm_f32(self.width, self.embed_dim, batch, pooled, 1, self.width, dfeat, self.embed_dim, 1, g,
                         self.embed_dim, 1.0, beta)
        else:
            dy = ops.cast_f32_bf16(dfeat, torch.empty(dfeat.shape, dtype=torch.bfloat16, device=dev))
            # dpooled[b,width] = dy[b,E] . proj^T  -> NT GEMM against the [width, E] copy (= W(name))
            dpooled = ops.linear_dgrad(dy, None, self.W(proj_name))
            # dproj[width,E] = pooled^T . dy
            ws_wg = self._workspace("wgrad", ops.linear_wgrad_ws_bytes(self.dtype, batch, self.width, self.embed_dim), dev)
            ops.linear_wgrad(pooled, dy, g, beta, ws_wg)
        if dtok_all is not None:
            # token outputs in use: the pooled rows are rows of the same LayerNorm output, so their gradient is added
            # into the dense token gradient and ONE dense LayerNorm backward handles both (glue: a [batch, width] index_add)
            g_all = dtok_all[:M].contiguous()
            g_all.index_add_(0, idx.long(), dpooled.to(g_all.dtype))
            dx = ops.layernorm_bwd(g_all, x_last, P[ln_name + ".weight"], mean_all, rstd_all, ws_ln)
        elif pruned:
            # x_last holds the pooled rows only: a compact [batch, width] gradient, no zero fill of the hidden state
            dx = ops.layernorm_bwd(dpooled, x_last, P[ln_name + ".weight"], meanp, rstdp, ws_ln)
        else:
            # pooled LayerNorm: scatter rows into a zero gradient of the last hidden state
            dx = torch.zeros_like(x_last)
            ops.layernorm_bwd(dpooled, x_last, P[ln_name + ".weight"], meanp, rstdp, ws_ln, dx_out=dx, row_index=idx)
        last_bias = f"transformer.resblocks.{self.layers - 1}.mlp.c_proj.bias" if self.layers > 0 else None
        self._ln_finish(ws_ln, self.width, ln_name + ".weight", ln_name + ".bias", last_bias)
        layout = head[1] if self.kind == "text" else None
        for i in reversed(range(self.layers)):
            sv = blocks[i]
            last_pruned = pruned and i == self.layers - 1
            if len(sv) == 1:          # a checkpointed block: only its input was kept
                _, sv = (self._block_fwd_pooled(sv[0], i, batch, L, layout, idx) if last_pruned
                         else self._block_fwd(sv[0], i, batch, L, layout, need_out=False))
            prev_bias = f"transformer.resblocks.{i - 1}.mlp.c_proj.bias" if i > 0 else None
            if last_pruned:
                dx = self._block_bwd_pooled(dx, sv, i, batch, L, prev_bias, layout, idx)
            else:
                dx = self._block_bwd(dx, sv, i, batch, L, prev_bias, layout)
            blocks[i] = None
            step = max(1, -(-self.layers // max(1, self.grad_chunks)))
            if i > 0 and (self.layers - i) % step == 0:
                self._grads_ready(i)
        if self.kind == "vision":
            patches, x0, mean0, rstd0, keep_idx = head
            dx0 = ops.layernorm_bwd(dx, x0, P["ln_pre.weight"], mean0, rstd0, ws_ln)
            self._ln_finish(ws_ln, self.width, "ln_pre.weight", "ln_pre.bias", None)
            gpos, bpos = self.G("positional_embedding")
            gcls, bcls = self.G("class_embedding")
            assert bpos == bcls
            if keep_idx is None:
                dtok = ops.vision_assemble_bwd(dx0, batch, self.seq, gpos, gcls, bpos)
            else:
                dtok = ops.vision_assemble_keep_bwd(dx0, keep_idx, self.seq - 1, gpos, gcls, bpos)
            self.owner.conv_wgrad(self, dtok, patches)
        else:
            text, layout = head
            gtab, btab = self.G("token_embedding.weight")
            if btab == 0.0:
                gtab.zero_()
            gpos, bpos = self.G("positional_embedding")
            if layout is not None:
                ops.text_embed_packed_bwd(layout, dx, gtab, gpos, bpos)
            else:
                ops.text_embed_bwd(text, dx, gtab, gpos, bpos)
        return self._finish_grads()


def _apply_tower(fn, engine, inp, params):
    """Run a tower node.  Inside `Function.forward` grad mode is always off and `ctx.needs_input_grad` stays True for parameters
    even under `torch.no_grad()`, so whether a backward can follow is read HERE: without it an evaluation / feature-caching pass
    would keep every block's activations (and write the pre-activations) like a training forward."""
    engine._grad_mode = torch.is_grad_enabled()
    return fn.apply(engine, inp, *params)


class _TowerFn(torch.autograd.Function):
    """One autograd node per tower: forward/backward are sequences of HIP kernel launches."""

    @staticmethod
    def forward(ctx, engine: _Engine, inp: torch.Tensor, *params: torch.Tensor):
        if not inp.is_cuda:
            raise RuntimeError("colxlip_amd: the model runs on MI355X only (no CPU fallback); move inputs to cuda")
        engine.bind(dict(zip(engine.names, params)))
        need = any(ctx.needs_input_grad[2:]) and getattr(engine, "_grad_mode", True)
        with phase(engine.kind + ".fwd"):
            feat, saved = engine.forward(inp.contiguous(), save=need)
        ctx.engine, ctx.saved_state = engine, saved
        if need:
            engine._open_backwards = getattr(engine, "_open_backwards", 0) + 1
        return feat

    @staticmethod
    def backward(ctx, dfeat):
        engine = ctx.engine
        with phase(engine.kind + ".bwd"):
            grads = engine.backward(ctx.saved_state, dfeat)
        ctx.saved_state = None
        engine._open_backwards = max(0, getattr(engine, "_open_backwards", 1) - 1)
        return (None, None, *grads)


class _TowerTokFn(torch.autograd.Function):
    """Tower node that also returns the final-LayerNorm'd token matrix [M + 1, width] (ColXLIP)."""

    @staticmethod
    def forward(ctx, engine: _Engine, inp: torch.Tensor, *params: torch.Tensor):
        if not inp.is_cuda:
            raise RuntimeError("colxlip_amd: the model runs on MI355X only (no CPU fallback); move inputs to cuda")
        engine.bind(dict(zip(engine.names, params)))
        need = any(ctx.needs_input_grad[2:]) and getattr(engine, "_grad_mode", True)
        feat, saved, tok_all = engine.forward(inp.contiguous(), save=need, want_tokens=True)
        ctx.engine, ctx.saved_state = engine, saved
        if need:
            engine._open_backwards = getattr(engine, "_open_backwards", 0) + 1
        return feat, tok_all

    @staticmethod
    def backward(ctx, dfeat, dtok_all):
        engine = ctx.engine
        grads = engine.backward(ctx.saved_state, dfeat, dtok_all)
        ctx.saved_state = None
        engine._open_backwards = max(0, getattr(engine, "_open_backwards", 1) - 1)
        return (None, None, *grads)


class _TokenHeadFn(torch.autograd.Function):
    """ColXLIP token projection (reference model.py:514-526): LayerNorm -> Linear -> GELU -> LayerNorm on the rows of
    `tok_all` selected by `row_index` (vision: every patch token; text: positions before EOT, the rest read the zero
    row).  Sequence of HIP kernel launches; returns [R, embed] in the compute dtype."""

    @staticmethod
    def forward(ctx, tok_all, row_index, ln1_w, ln1_b, lin_w, lin_b, ln2_w, ln2_b):
        dt = tok_all.dtype
        R = row_index.shape[0]
        h1, mean1, rstd1 = ops.layernorm_fwd(tok_all, ln1_w, ln1_b, rows=R, row_index=row_index)
        if dt == torch.float32:
            w16 = wt16 = None
            a, u = ops.linear_fwd(h1, lin_w, lin_b, act=ACT_GELU, want_preact=True)
        else:
            w16 = torch.empty(lin_w.shape, dtype=torch.bfloat16, device=lin_w.device)
            wt16 = torch.empty((lin_w.shape[1], lin_w.shape[0]), dtype=torch.bfloat16, device=lin_w.device)
            ops.cast_weight(lin_w.detach(), w16, wt16)
            a, u = ops.linear_fwd(h1, w16, lin_b, act=ACT_GELU, want_preact=True)
        h2, mean2, rstd2 = ops.layernorm_fwd(a, ln2_w, ln2_b)
        ctx.save_for_backward(tok_all, row_index, ln1_w, lin_w, ln2_w, h1, mean1, rstd1, u, a, mean2, rstd2,
                              wt16 if wt16 is not None else lin_w)
        return h2

    @staticmethod
    def backward(ctx, dh2):
        tok_all, row_index, ln1_w, lin_w, ln2_w, h1, mean1, rstd1, u, a, mean2, rstd2, wt16 = ctx.saved_tensors
        dt = tok_all.dtype
        dev = tok_all.device
        E, width = lin_w.shape
        R = h1.shape[0]
        dh2 = dh2.contiguous().to(dt)
        ws2 = torch.empty((ops.layernorm_ws_bytes(E),), dtype=torch.uint8, device=dev)
        da = ops.layernorm_bwd(dh2, a, ln2_w, mean2, rstd2, ws2)
        g_ln2_w, g_ln2_b = torch.empty_like(ln2_w), torch.empty_like(ln2_w)
        ops.layernorm_bwd_finish(E, ws2, g_ln2_w, None, None, 0.0)
        ops.layernorm_bwd_finish(E, ws2, None, g_ln2_b, None, 0.0)
        g_lin_b = torch.empty((E,), dtype=torch.float32, device=dev)
        ws_cs = torch.empty((ops.colsum_ws_bytes(R, E),), dtype=torch.uint8, device=dev)
        du = ops.act_bwd_colsum(da, u, ACT_GELU, g_lin_b, 0.0, ws_cs)            # du = da * GELU'(u), bias grad
        g_lin_w = torch.empty((E, width), dtype=torch.float32, device=dev)
        ws_wg = torch.empty((max(ops.linear_wgrad_ws_bytes(dt, R, E, width), 16),), dtype=torch.uint8, device=dev)
        ops.linear_wgrad(du, h1, g_lin_w, 0.0, ws_wg)
        dh1 = ops.linear_dgrad(du, lin_w if dt == torch.float32 else None, None if dt == torch.float32 else wt16)
        ws1 = torch.empty((ops.layernorm_ws_bytes(width),), dtype=torch.uint8, device=dev)
        dtok_all = torch.zeros_like(tok_all)
        ops.layernorm_bwd(dh1, tok_all, ln1_w, mean1, rstd1, ws1, dx_out=dtok_all, row_index=row_index)
        g_ln1_w, g_ln1_b = torch.empty_like(ln1_w), torch.empty_like(ln1_w)
        ops.layernorm_bwd_finish(width, ws1, g_ln1_w, None, None, 0.0)
        ops.layernorm_bwd_finish(width, ws1, None, g_ln1_b, None, 0.0)
        return dtok_all, None, g_ln1_w, g_ln1_b, g_lin_w, g_lin_b, g_ln2_w, g_ln2_b


class _L2NormFn(torch.autograd.Function):
    """F.normalize(x, dim=-1) (reference model.py:552,606)."""

    @staticmethod
    def forward(ctx, x):
        y, inv = ops.l2norm_fwd(x.contiguous())
        ctx.save_for_backward(y, inv)
        return y

    @staticmethod
    def backward(ctx, dy):
        y, inv = ctx.saved_tensors
        return ops.l2norm_bwd(dy.contiguous(), y, inv)


def l2_normalize(x: torch.Tensor) -> torch.Tensor:
    return _L2NormFn.apply(x)


# --------------------------------------------------------------------------- towers
def _to_2tuple(x):
    return tuple(x) if isinstance(x, (tuple, list)) else (x, x)


class PatchDropout(nn.Module):
    """Patch dropout (FLIP, arXiv 2212.00794; reference transformer.py:48-88 with exclude_first_token=True, as its
    VisionTransformer builds it).  A control object without parameters or buffers (the state dict is unchanged): while the image
    tower is in training mode and prob > 0, every forward draws which `num_keep(G2)` patch tokens of each image are kept, and the
    tower's kernels run on those (the class token always stays); otherwise nothing of it runs.

    rng="device" (default): one 63-bit key per forward from torch's default CPU generator (so masks follow the seed; no device
    sync), expanded on the device by clipx_patch_keep_index: uniform without replacement, ascending.  The same distribution as
    the reference's, not its random stream.
    rng="torch": the reference's own draw, `torch.randn(batch, G2).topk(keep).indices` on the CPU, copied to the device
    (parity / reproduction mode)."""

    def __init__(self, prob: float = 0.5, exclude_first_token: bool = True, rng: str = "device"):
        super().__init__()
        if not (0 <= prob < 1.0):
            raise ValueError(f"patch dropout probability must be in [0, 1), got {prob}")
        if not exclude_first_token:
            raise NotImplementedError("patch dropout without exclude_first_token is not supported (no config reaches it)")
        self.prob = float(prob)
        self.exclude_first_token = True
        self.rng = rng
        self._last_keep_index = None

    @property
    def rng(self) -> str:
        return self._rng

    @rng.setter
    def rng(self, value: str):
        if value not in ("device", "torch"):
            raise ValueError(f"patch dropout rng must be 'device' or 'torch', got {value!r}")
        self._rng = value

    def num_keep(self, G2: int) -> int:
        """reference transformer.py:76-77, in Python float: p = 0.9, G2 = 20 keeps 1"""
        return max(1, int(G2 * (1 - self.prob)))

    @property
    def last_keep_index(self) -> Optional[torch.Tensor]:
        """int32 [batch, keep] on the device: the mask of the last training-mode forward (None before the first)"""
        return self._last_keep_index

    def draw(self, batch: int, G2: int, device) -> torch.Tensor:
        keep = self.num_keep(G2)
        if self.rng == "torch":
            # glue: the reference's CPU draw, byte for byte (transformer.py:79-80)
            idx = torch.randn(batch, G2).topk(keep, dim=-1).indices.to(torch.int32).to(device)
        else:
            key = int(torch.randint(0, 2 ** 63 - 1, (1,), dtype=torch.int64))
            idx = ops.patch_keep_index(batch, G2, keep, key, device)
        self._last_keep_index = idx
        return idx

    def extra_repr(self) -> str:
        return f"prob={self.prob}, rng={self.rng!r}"


class VisionTransformer(nn.Module):
    """Image tower (reference transformer.py:515-836, 'tok' pooling, learnable pos-embed)."""

    def __init__(self, image_size, patch_size: int, width: int, layers: int, heads: int, mlp_ratio: float,
                 output_dim: int, act: int = ACT_GELU, patch_dropout: float = 0.0):
        super().__init__()
        self.image_size = _to_2tuple(image_size)
        self.patch_size = _to_2tuple(patch_size)
        self.grid_size = (self.image_size[0] // self.patch_size[0], self.image_size[1] // self.patch_size[1])
        self.output_dim = output_dim
        self.output_tokens = False
        scale = width ** -0.5
        self.class_embedding = nn.Parameter(scale * torch.randn(width))
        self.positional_embedding = nn.Parameter(scale * torch.randn(self.grid_size[0] * self.grid_size[1] + 1, width))
        self.proj = nn.Parameter(scale * torch.randn(width, output_dim))
        self.conv1 = ConvParams(width, self.patch_size[0])
        self.ln_pre = LayerNormParams(width)
        self.transformer = Transformer(width, layers, heads, mlp_ratio)
        self.ln_post = LayerNormParams(width)
        self.patch_dropout = PatchDropout(patch_dropout)
        self._names = [n for n, _ in self.named_parameters()]
        seq = self.grid_size[0] * self.grid_size[1] + 1
        self._engine = _Engine("vision", self, self.transformer, seq, False, act, output_dim, self._names)
        self._conv16 = None

    def k_padded(self, dtype) -> int:
        k = 3 * self.patch_size[0] * self.patch_size[1]
        return k if dtype == torch.float32 else (k + 63) // 64 * 64

    def conv_shadow(self, engine: _Engine):
        """bf16 [width, Kp] copy of conv1.weight (K zero-padded to a multiple of 64)."""
        p = self.conv1.weight
        ent = self._conv16
        if ent is None or ent[1] != p._version or ent[2] != p.data_ptr():
            w = p.detach().view(p.shape[0], -1)
            kp = self.k_padded(torch.bfloat16)
            if kp == w.shape[1]:
                w16 = torch.empty((w.shape[0], kp), dtype=torch.bfloat16, device=w.device)
                ops.cast_weight(w, w16, None)
            else:
                w16 = torch.zeros((w.shape[0], kp), dtype=torch.bfloat16, device=w.device)
                w16[:, :w.shape[1]] = w    # rare (patch 14): host-side pad, once per weight update
            ent = (w16, p._version, p.data_ptr())
            self._conv16 = ent
        return ent[0]

    def conv_wgrad(self, engine: _Engine, dtok, patches):
        g, beta = engine.G("conv1.weight")
        K = 3 * self.patch_size[0] * self.patch_size[1]
        M, width = dtok.shape
        kp = patches.shape[1]
        dev = dtok.device
        ws = engine._workspace("wgrad", ops.linear_wgrad_ws_bytes(engine.dtype, M, width, kp), dev)
        if kp == K:
            ops.linear_wgrad(dtok, patches, g.view(width, K), beta, ws)
        else:
            tmp = torch.empty((width, kp), dtype=torch.float32, device=dev)
            ops.linear_wgrad(dtok, patches, tmp, 0.0, ws)
            gv = g.view(width, K)
            if beta == 0.0:
                gv.copy_(tmp[:, :K])
            else:
                gv.add_(tmp[:, :K])

    def set_grad_checkpointing(self, enable: bool = True):
        self.transformer.grad_checkpointing = enable

    def forward(self, x: torch.Tensor):
        return _apply_tower(_TowerFn, self._engine, x, [p for _, p in self.named_parameters()])


class CLIP(nn.Module):
    """open_clip.model.CLIP contract (third-party in the reference; see module docstring)."""

    output_dict: bool

    def __init__(self, embed_dim: int, vision_cfg, text_cfg, quick_gelu: bool = False,
                 init_logit_scale: float = math.log(1 / 0.07), init_logit_bias: Optional[float] = None,
                 cast_dtype: Optional[torch.dtype] = None, output_dict: bool = False, precision: str = "fp32"):
        super().__init__()
        if isinstance(vision_cfg, dict):
            vision_cfg = CLIPVisionCfg(**vision_cfg)
        if isinstance(text_cfg, dict):
            text_cfg = CLIPTextCfg(**text_cfg)
        for flag, val in (("attentional_pool", vision_cfg.attentional_pool), ("timm_model_name", vision_cfg.timm_model_name),
                          ("hf_model_name", text_cfg.hf_model_name), ("embed_cls", text_cfg.embed_cls),
                          ("no_causal_mask", text_cfg.no_causal_mask), ("ls_init_value", vision_cfg.ls_init_value)):
            if val:
                raise NotImplementedError(f"{flag} is outside the MI355X hot path (plain ViT + text transformer CLIP)")
        self.output_dict = output_dict
        self.precision = precision
        act = ACT_QUICKGELU if quick_gelu else ACT_GELU
        self.visual = VisionTransformer(vision_cfg.image_size, vision_cfg.patch_size, vision_cfg.width,
                                        vision_cfg.layers, vision_cfg.width // vision_cfg.head_width,
                                        vision_cfg.mlp_ratio, embed_dim, act, patch_dropout=vision_cfg.patch_dropout or 0.0)
        # text tower parameters live at top level (reference model.py:569-599)
        self.context_length = text_cfg.context_length
        self.vocab_size = text_cfg.vocab_size
        self.text_pool_type = text_cfg.pool_type
        dt = text_cfg.width
        self.transformer = Transformer(dt, text_cfg.layers, text_cfg.heads, text_cfg.mlp_ratio)
        self.token_embedding = nn.Embedding(text_cfg.vocab_size, dt)
        self.positional_embedding = nn.Parameter(torch.empty(text_cfg.context_length, dt))
        self.ln_final = LayerNormParams(dt)
        self.text_projection = nn.Parameter(torch.empty(dt, embed_dim))
        self.register_buffer("attn_mask", torch.triu(torch.full((text_cfg.context_length,) * 2, float("-inf")), 1),
                             persistent=False)
        self.logit_scale = nn.Parameter(torch.ones([]) * init_logit_scale)
        self.logit_bias = nn.Parameter(torch.ones([]) * init_logit_bias) if init_logit_bias is not None else None
        self._init_text_parameters()
        self._text_names = [n for n, _ in self.named_parameters()
                            if not n.startswith("visual.") and n not in ("logit_scale", "logit_bias")]
        self._text_engine = _Engine("text", self, self.transformer, text_cfg.context_length, True, act, embed_dim,
                                    self._text_names)
        self._text_engine.peer, self.visual._engine.peer = self.visual._engine, self._text_engine
        self.set_precision(precision)

    def _init_text_parameters(self):
        """reference transformer.py:925-946"""
        tf = self.transformer
        nn.init.normal_(self.token_embedding.weight, std=0.02)
        nn.init.normal_(self.positional_embedding, std=0.01)
        proj_std = (tf.width ** -0.5) * ((2 * tf.layers) ** -0.5)
        attn_std = tf.width ** -0.5
        fc_std = (2 * tf.width) ** -0.5
        for blk in tf.resblocks:
            nn.init.normal_(blk.attn.in_proj_weight, std=attn_std)
            nn.init.normal_(blk.attn.out_proj.weight, std=proj_std)
            nn.init.normal_(blk.mlp.c_fc.weight, std=fc_std)
            nn.init.normal_(blk.mlp.c_proj.weight, std=proj_std)
        nn.init.normal_(self.text_projection, std=tf.width ** -0.5)

    # -- DistributedDataParallel wrap (reference main.py:264-271 wraps whatever the factory returns) --------------
    @property
    def _ddp_params_and_buffers_to_ignore(self):
        """Read by DistributedDataParallel.__init__.  The towers' parameter gradients live in two flat arenas that this
        stack averages itself (distributed.GradSync, in place, overlapped with the backward); handing them to DDP's
        reducer as well would copy 605 MB into 25 MB buckets and back every step.  So DDP is told to ignore the tower
        parameters (and the constant causal-mask buffer it would otherwise re-broadcast every forward); it keeps
        `logit_scale` / `logit_bias` (and ColXLIP's token heads).  Being asked is the signal that a DDP wrapper is being
        built: from then on every backward averages the arenas across the default process group by itself."""
        object.__setattr__(self, "_auto_sync_requested", True)
        names = ["visual." + n for n in self.visual._names] + list(self._text_names) + ["attn_mask"]
        # DDP matches the names two ways: `named_parameters()` names for its parameter broadcast, but f"{module_name}.{name}"
        # when it builds the reducer's parameter list -- which for a parameter held DIRECTLY by the wrapped module
        # (positional_embedding, text_projection, the attn_mask buffer) is ".positional_embedding".  With only the plain name
        # the reducer kept those two: it all-reduced them a second time and, in an accumulating backward (where this stack adds
        # in place and no AccumulateGrad fires), copied its stale bucket back over the gradient -- found by
        # tests/test_dist_gpu.py::test_ddp_wrapped_model_matches_plain run after another test.  Both spellings are listed.
        return names + ["." + n for n in names if "." not in n]

    def _maybe_auto_sync(self):
        if not getattr(self, "_auto_sync_requested", False) or getattr(self, "_auto_sync", None) is not None:
            return
        import torch.distributed as dist
        if not (dist.is_available() and dist.is_initialized()):
            return
        force = os.environ.get("CLIPX_FORCE_SYNC", "0") == "1"       # 1-rank RCCL rehearsal on a one-GPU box
        world = dist.get_world_size()
        if world <= 1 and not force:
            return
        from .distributed import GradSync
        own = dict(self.named_parameters())
        names = ["visual." + n for n in self.visual._names] + list(self._text_names)
        gs = GradSync([own[n] for n in names], world, force=force, fence_in_backward=True)
        if self.visual._engine.grad_ready_hook is None and self._text_engine.grad_ready_hook is None:
            gs.attach(self)
        object.__setattr__(self, "_auto_sync", gs)

    # -- precision ---------------------------------------------------------------------------
    def set_precision(self, precision: str):
        self.precision = precision
        cd = compute_dtype_for(precision)
        for eng in (self.visual._engine, self._text_engine):
            eng.dtype = cd
            eng.weight_quant = "e4m3" if precision in ("fp8", "fp8_mfma") else None
            eng.act_quant = "e4m3" if precision == "fp8_mfma" else None
            eng._shadow.clear()
            eng._quant_key = eng._cast_key = None       # descriptor tables point into the copies just dropped

    def export_fp8_weights(self):
        """{parameter name: (e4m3 bytes [N, K] uint8, per-row exponents [N] int32)} of the quantised block weights as of
        the last forward (precision 'fp8'): value = e4m3 * 2**exponent."""
        out = {}
        for prefix, eng in (("visual.", self.visual._engine), ("", self._text_engine)):
            for name, ent in eng._shadow.items():
                if len(ent) >= 6 and ent[4] is not None:
                    out[prefix + name] = (ent[4], ent[5])
        return out

    @property
    def compute_dtype(self) -> torch.dtype:
        return self._text_engine.dtype

    def set_grad_checkpointing(self, enable: bool = True):
        self.visual.set_grad_checkpointing(enable)
        self.transformer.grad_checkpointing = enable

    # -- forward ------------------------------------------------------------------------------
    def encode_image(self, image, normalize: bool = False):
        features = self.visual(image)
        return l2_normalize(features) if normalize else features

    def encode_text(self, text, normalize: bool = False):
        params = dict(self.named_parameters())
        features = _apply_tower(_TowerFn, self._text_engine, text, [params[n] for n in self._text_names])
        return l2_normalize(features) if normalize else features

    def get_logits(self, image, text):
        image_features = self.encode_image(image, normalize=True)
        text_features = self.encode_text(text, normalize=True)
        from .loss import _ScaledMatmul                       # the fp32 HIP GEMM (with its backward), not a library matmul
        image_logits = _ScaledMatmul.apply(image_features, text_features, self.logit_scale.exp())
        if self.logit_bias is not None:
            image_logits = image_logits + self.logit_bias
        return image_logits, image_logits.T

    def _tower_streams(self, device):
        """Two side HIP streams, one per tower (env CLIPX_TOWER_STREAMS=0 turns them off)."""
        if os.environ.get("CLIPX_TOWER_STREAMS", "1") == "0":
            return None
        st = getattr(self, "_side_streams", None)
        if st is None or st[0].device != device:
            st = (torch.cuda.Stream(device=device), torch.cuda.Stream(device=device))
            object.__setattr__(self, "_side_streams", st)
        return st

    def forward(self, image: Optional[torch.Tensor] = None, text: Optional[torch.Tensor] = None):
        self._maybe_auto_sync()
        streams = self._tower_streams(image.device) if (image is not None and text is not None and image.is_cuda) else None
        if streams is not None:
            # The towers are independent until the loss: each runs on its own HIP stream (autograd replays a node's
            # backward on the stream its forward ran on, so the two backwards overlap as well).  Every GEMM here is a
            # persistent one-block-per-CU kernel whose last round of tiles leaves CUs idle -- at per-GPU batch 512
            # that is 20-40 % of a launch -- and the other tower's kernels fill exactly those CUs.
            main = torch.cuda.current_stream(image.device)
            s_img, s_txt = streams
            s_img.wait_stream(main)
            s_txt.wait_stream(main)
            with torch.cuda.stream(s_img):
                image_features = self.encode_image(image, normalize=True)
            with torch.cuda.stream(s_txt):
                text_features = self.encode_text(text, normalize=True)
            main.wait_stream(s_img)
            main.wait_stream(s_txt)
            image.record_stream(s_img)
            text.record_stream(s_txt)
            image_features.record_stream(main)
            text_features.record_stream(main)
        else:
            image_features = self.encode_image(image, normalize=True) if image is not None else None
            text_features = self.encode_text(text, normalize=True) if text is not None else None
        if self.output_dict:
            out = {"image_features": image_features, "text_features": text_features,
                   "logit_scale": self.logit_scale.exp()}
            if self.logit_bias is not None:
                out["logit_bias"] = self.logit_bias
            return out
        if self.logit_bias is not None:
            return image_features, text_features, self.logit_scale.exp(), self.logit_bias
        return image_features, text_features, self.logit_scale.exp()


# --------------------------------------------------------------------------- ColXLIP ("next" row)
class TokenHeadParams(nn.Module):
    """Parameter layout of the reference's nn.Sequential(LayerNorm, Linear, GELU, LayerNorm) (model.py:514-526):
    state-dict keys `<name>.0.*`, `<name>.1.*`, `<name>.3.*`."""

    def __init__(self, width: int, embed_dim: int):
        super().__init__()
        self.add_module("0", LayerNormParams(width))
        self.add_module("1", LinearParams(width, embed_dim))
        self.add_module("3", LayerNormParams(embed_dim))

    def tensors(self):
        m = dict(self.named_children())
        return (m["0"].weight, m["0"].bias, m["1"].weight, m["1"].bias, m["3"].weight, m["3"].bias)


class ColXLIP(CLIP):
    """reference model.py:455-687: CLIP + ColBERT-style token features.  forward() returns the reference's dict
    (image_features, text_features, token_image_features [b, Lv-1, E], token_text_features [b, 77, E], logit_scale);
    text token positions at and after EOT are zeroed BEFORE the token head, exactly as the reference does."""

    def __init__(self, embed_dim: int, vision_cfg, text_cfg, quick_gelu: bool = False,
                 init_logit_scale: float = math.log(1 / 0.07), init_logit_bias: Optional[float] = None,
                 cast_dtype: Optional[torch.dtype] = None, output_dict: bool = True, alpha: float = 0.5,
                 precision: str = "fp32"):
        pd = vision_cfg.get("patch_dropout") if isinstance(vision_cfg, dict) else getattr(vision_cfg, "patch_dropout", 0.0)
        if pd and pd > 0:
            raise NotImplementedError("patch_dropout is not supported for ColXLIP: its token MaxSim path reads every patch token")
        super().__init__(embed_dim, vision_cfg, text_cfg, quick_gelu=quick_gelu, init_logit_scale=init_logit_scale,
                         init_logit_bias=init_logit_bias, cast_dtype=cast_dtype, output_dict=True, precision=precision)
        self.alpha = alpha
        self.vision_token_layer = TokenHeadParams(self.visual.transformer.width, embed_dim)
        self.text_token_layer = TokenHeadParams(self.transformer.width, embed_dim)
        self._idx_cache = {}

    def _text_tower_names(self):
        # the text engine owns only the tower's parameters, not the token heads
        return [n for n in self._text_names]

    def _vision_rows(self, batch: int, device):
        key = ("v", batch, device)
        if key not in self._idx_cache:
            L = self.visual._engine.seq
            base = torch.arange(batch, device=device, dtype=torch.int32).unsqueeze(1) * L
            self._idx_cache[key] = (base + torch.arange(1, L, device=device, dtype=torch.int32)).reshape(-1).contiguous()
        return self._idx_cache[key]

    def encode_image(self, image, normalize: bool = False):
        eng = self.visual._engine
        feat, tok_all = _apply_tower(_TowerTokFn, eng, image, [p for _, p in self.visual.named_parameters()])
        batch = image.shape[0]
        rows = self._vision_rows(batch, image.device)
        tokens = _TokenHeadFn.apply(tok_all, rows, *self.vision_token_layer.tensors())
        if normalize:
            feat = l2_normalize(feat)
            tokens = l2_normalize(tokens.float()).to(tokens.dtype)
        return feat, tokens.view(batch, eng.seq - 1, -1)

    def encode_text(self, text, normalize: bool = False):
        eng = self._text_engine
        params = dict(self.named_parameters())
        feat, tok_all = _apply_tower(_TowerTokFn, eng, text, [params[n] for n in self._text_names])
        batch, L = text.shape
        # positions before the pooled (EOT = arg-max id) token keep their features, the rest read the zero row
        # (reference model.py:578-591); integer index glue only
        pos = torch.arange(L, device=text.device, dtype=torch.int32).unsqueeze(0)
        layout = eng.last_layout
        M = tok_all.shape[0] - 1                                   # index of the zero row
        if layout is not None:                                     # packed rows: caption s, position t -> cu[s] + t
            cu = layout.cu[:batch + 1]
            base = cu[:batch].unsqueeze(1)
            eot = (cu[1:batch + 1] - cu[:batch] - 1).unsqueeze(1)
        else:
            base = torch.arange(batch, device=text.device, dtype=torch.int32).unsqueeze(1) * L
            eot = text.argmax(dim=-1).to(torch.int32).unsqueeze(1)
        rows = torch.where(pos < eot, base + pos, torch.full_like(base + pos, M)).reshape(-1).contiguous()
        tokens = _TokenHeadFn.apply(tok_all, rows, *self.text_token_layer.tensors())
        if normalize:
            feat = l2_normalize(feat)
            tokens = l2_normalize(tokens.float()).to(tokens.dtype)
        return feat, tokens.view(batch, L, -1)

    def get_logits(self, image, text, alpha: Optional[float] = None):
        """(logits_per_image [B_i, B_t], logits_per_text): logit_scale.exp() * (alpha * I T^T + (1 - alpha) * MaxSim(tokens)^T),
        the scoring the reference's forward carries as a commented-out block (model.py:670-685); `alpha` defaults to self.alpha.
        With grad enabled it is composed of the differentiable pieces the loss uses; under no_grad it is `ops.maxsim_scores`."""
        alpha = self.alpha if alpha is None else float(alpha)
        image_features, token_image_features = self.encode_image(image, normalize=True)
        text_features, token_text_features = self.encode_text(text, normalize=True)
        if not torch.is_grad_enabled():
            from .train import similarity_matrix
            image_logits = ops.maxsim_scores(token_image_features, token_text_features,
                                             similarity_matrix(image_features, text_features), alpha,
                                             float(self.logit_scale.exp()))
        else:
            from .loss import _ScaledMatmul, compute_colbert_similarity
            scale = self.logit_scale.exp()
            image_logits = _ScaledMatmul.apply(image_features, text_features, scale)
            if alpha != 1.0:
                token_logits = scale * compute_colbert_similarity(token_image_features, token_text_features).T
                image_logits = alpha * image_logits + (1 - alpha) * token_logits
        if self.logit_bias is not None:
            image_logits = image_logits + self.logit_bias
        return image_logits, image_logits.T

    def forward(self, image: Optional[torch.Tensor] = None, text: Optional[torch.Tensor] = None, alpha: Optional[float] = None):
        if image is None and text is None:
            return {}
        self._maybe_auto_sync()
        image_features, token_image_features = self.encode_image(image, normalize=True) if image is not None else (None, None)
        text_features, token_text_features = self.encode_text(text, normalize=True) if text is not None else (None, None)
        out = {"image_features": image_features, "text_features": text_features,
               "token_image_features": token_image_features, "token_text_features": token_text_features,
               "logit_scale": self.logit_scale.exp()}
        if self.logit_bias is not None:
            out["logit_bias"] = self.logit_bias
        return out


# --------------------------------------------------------------------------- preprocess cfg helpers
def get_model_preprocess_cfg(model):
    """reference model.py:421-435"""
    module = getattr(model, "visual", model)
    preprocess_cfg = getattr(module, "preprocess_cfg", {})
    if not preprocess_cfg:
        size = getattr(module, "image_size")
        if size is not None:
            preprocess_cfg["size"] = size
        for k in ("mean", "std"):
            v = getattr(module, "image_" + k, None)
            if v is not None:
                preprocess_cfg[k] = v
    return preprocess_cfg


def set_model_preprocess_cfg(model, preprocess_cfg: Dict[str, Any]):
    """reference model.py:438-442"""
    module = getattr(model, "visual", model)
    module.image_mean = preprocess_cfg["mean"]
    module.image_std = preprocess_cfg["std"]
    module.preprocess_cfg = copy.deepcopy(preprocess_cfg)


def get_model_tokenize_cfg(model):
    """{context_length, vocab_size} of the text tower (reference model.py `get_model_tokenize_cfg`, exported by the package)."""
    cfg = {}
    for key in ("context_length", "vocab_size"):
        val = getattr(model, key, None)
        if val is not None:
            cfg[key] = val
    return cfg


# --------------------------------------------------------------------------- low-precision weights
def lp_parameter_names(model: nn.Module) -> List[str]:
    """Names of the parameters the reference's `convert_weights_to_lp` casts (model.py:228-255): weight and bias of every
    Linear / Conv (here: LinearParams, ConvParams, the token heads' nn.Linear), the packed attention in-projection, and the two
    projection matrices `text_projection` / `visual.proj`.  LayerNorm parameters, embeddings, class / position embeddings and
    `logit_scale` stay fp32 there (LayerNormFp32, model.py:146,201) and are not listed."""
    names = []
    for mod_name, mod in model.named_modules():
        dot = mod_name + "." if mod_name else ""
        if isinstance(mod, (LinearParams, ConvParams, nn.Linear)):
            names += [dot + n for n in ("weight", "bias") if getattr(mod, n, None) is not None]
        elif isinstance(mod, AttentionParams):
            names += [dot + "in_proj_weight", dot + "in_proj_bias"]
        if isinstance(mod, CLIP):
            names.append(dot + "text_projection")
        if isinstance(mod, VisionTransformer) and getattr(mod, "proj", None) is not None:
            names.append(dot + "proj")
    return names


_LP_TOLD = set()


def convert_weights_to_lp(model: nn.Module, dtype=torch.float16):
    """Reference model.py:228-255 under this stack's storage model.  There, the listed tensors are REPLACED by `dtype`
    tensors.  Here every parameter stays an fp32 master (the kernels read bf16 operand copies made from the masters, Adam
    moments are fp32), so the cast is applied to the VALUES: each listed tensor is rounded in place to the nearest `dtype`
    value -- after the call the model holds exactly the numbers the reference's low-precision tensors would hold (and a
    state_dict saved from it loads bit-identically into a reference model in that precision) -- and a model still in the
    fp32 parity mode is switched to bf16 operands.  Only bfloat16 is supported (no fp16 kernels are built, see
    `compute_dtype_for`)."""
    if dtype in (torch.float16, "fp16"):
        raise NotImplementedError("convert_weights_to_lp(dtype=float16): this stack has no fp16 kernels (CDNA4 runs bf16 and fp16 "
                                  "MFMA at the same rate); pass dtype=torch.bfloat16")
    if dtype is not torch.bfloat16:
        raise ValueError(f"convert_weights_to_lp: unsupported dtype {dtype}")
    params = dict(model.named_parameters())
    with torch.no_grad():
        for name in lp_parameter_names(model):
            p = params[name]
            p.copy_(p.to(torch.bfloat16).to(p.dtype))        # copy_ bumps the version: stale operand copies are refreshed
    core = getattr(model, "module", model)
    if isinstance(core, CLIP) and core.compute_dtype == torch.float32:
        core.set_precision("bf16")
    if "lp" not in _LP_TOLD:
        _LP_TOLD.add("lp")
        import logging
        logging.warning("colxlip_amd: convert_weights_to_lp rounds the Linear / Conv / attention / projection parameters to bf16 "
                        "VALUES in place; storage stays fp32 (master weights), LayerNorm parameters are untouched")


convert_weights_to_fp16 = convert_weights_to_lp  # the reference's backwards-compat alias (model.py:258)


def trace_model(model, batch_size=256, device=torch.device('cpu')):
    raise NotImplementedError("trace_model: torchscript tracing is not supported (the towers are HIP kernel sequences behind "
                              "autograd.Function nodes)")
