"""Test helper of the late-interaction tests (test_late_interaction_*, test_maxsim_small_*, test_search_*, test_search_fp8_*): the
inputs they share, the reference's MaxSim arithmetic in torch, torch models of the e4m3 row quantiser and of the packed-row
count, and the small models the index is searched through.  Generators return fp32 CPU tensors unless they take a dtype; the
callers cast and move them.  It lives with the tests because the product has no CPU path."""
import itertools

import torch

from oracle import clip_oracle as O

Q49_MODEL = "ViT-q49-test-colxlip"      # 112 px / patch 16: 49 image tokens, embed dim 128
Q49 = O.ClipCfg(embed_dim=128, image_size=112, patch_size=16, vision_width=128, vision_layers=2,
                context_length=77, vocab_size=1024, text_width=128, text_heads=2, text_layers=2)

# `python -c LAUNCHER <repository root> <arguments of colxlip_amd.search>`: the command line with the tests' model configs
LAUNCHER = ("import os, sys; sys.path.insert(0, sys.argv[1]); from colxlip_amd import add_model_config; "
            "add_model_config(os.path.join(sys.argv[1], 'tests', 'model_configs')); from colxlip_amd.search import main; "
            "sys.exit(main(sys.argv[2:]))")


# ---- scorer inputs and reference ------------------------------------------------------------------------------------------
def tokens(ni, q, nt, n, e, seed=None, distinct=False):
    """(image tokens [ni, q, e], text tokens [nt, n, e]), normalised rows; seed 100 + q unless given.  The text is shaped like
    ColXLIP's output: every position at / behind a per-sample EOT is one vector, sample 1 has exact-zero rows there, sample 2
    keeps distinct rows to the end, and the last sample's EOT is 0: one packed row.  `distinct`: every other sample keeps
    distinct rows too (many packed rows from few samples)."""
    g = torch.Generator().manual_seed(100 + q if seed is None else seed)
    ti = torch.nn.functional.normalize(torch.randn(ni, q, e, generator=g), dim=-1)
    tt = torch.nn.functional.normalize(torch.randn(nt, n, e, generator=g), dim=-1)
    tail = torch.nn.functional.normalize(torch.randn(e, generator=g), dim=-1)
    for m in range(nt):
        eot = 2 + (5 * m) % (n - 2)
        if m == 1:
            tt[m, eot:] = 0.0
        elif m == nt - 1:
            tt[m, :] = tail
        elif m != 2 and not distinct:
            tt[m, eot:] = tail
    return ti, tt


def einsum_ref(ti, tt):
    """reference loss.py:20-46 in the dtype of its arguments (as tests/test_model_gpu.py:606-609 in fp32) -> tok [nt, ni]"""
    sim = torch.einsum('mnd,kqd->mknq', tt, ti)
    mx = sim.max(dim=3)[0]
    return mx.sum(-1) / ((mx != 0).to(mx.dtype).sum(-1) + 1e-8)


def shrink(monkeypatch, q, e, ci, rows, elem_bytes=2):
    """chunk limits under which the fused plan holds `ci` images of `elem_bytes`-byte elements per chunk and at most `rows`
    packed rows per text chunk"""
    from colxlip_amd import ops
    monkeypatch.setattr(ops, "MAXSIM_OPERAND_BYTES", ci * q * e * elem_bytes)
    monkeypatch.setattr(ops, "MAXSIM_TARGET_ROWS", rows)
    monkeypatch.setattr(ops, "MAXSIM_PARTIAL_BYTES", ops.maxsim_partial_bytes(ci, q, rows))


def cu_of(counts):
    """packed rows per sample -> their running sum [nt + 1], the `cu` of the chunk plan"""
    return [0] + list(itertools.accumulate(counts))


def packed_counts(nt, n, seed):
    """packed rows per sample: EOT-shaped lengths in [1, n], deterministic"""
    return [1 + (seed + 37 * m * m + 11 * m) % n for m in range(nt)]


# ---- index inputs ---------------------------------------------------------------------------------------------------------
def features(n, e, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.nn.functional.normalize(torch.randn(n, e, generator=g), dim=-1)


def image_tokens(n, q, e, seed, dtype=torch.bfloat16):
    g = torch.Generator().manual_seed(seed)
    return torch.nn.functional.normalize(torch.randn(n, q, e, generator=g), dim=-1).to(dtype)


def text_tokens(n, length, e, seed, dtype=torch.bfloat16):
    """EOT-shaped: every position at and behind a per-sample EOT holds one vector"""
    g = torch.Generator().manual_seed(seed)
    t = torch.nn.functional.normalize(torch.randn(n, length, e, generator=g), dim=-1)
    for m in range(n):
        eot = 2 + (5 * m) % (length - 2)
        t[m, eot:] = t[m, eot]
    return t.to(dtype)


# ---- models ---------------------------------------------------------------------------------------------------------------
def model_state(cfg, heads=True):
    """the oracle's perturbed state dict of `cfg`, with ColXLIP's token heads unless `heads` is False"""
    sd = O.perturb_state_dict(O.init_state_dict(cfg, seed=3), seed=4)
    if heads:
        sd.update(O.perturb_state_dict(O.init_colxlip_heads(cfg, seed=5), seed=6))
    return sd


def build_model(name, sd, precision, device="cuda"):
    from colxlip_amd import create_model_and_transforms
    model, _, _ = create_model_and_transforms(name, precision=precision, device=device, output_dict=True)
    model.load_state_dict({k: v.clone() for k, v in sd.items()}, strict=True)
    return model


# ---- torch models of the kernels an fp8 index is filled through --------------------------------------------------------------
def quant_model(x):
    """`clipx_quant_rows_e4m3` in torch: frexp(amax) = fr * 2^ex; e = ex - 9 if fr <= 0.875 else ex - 8 (the smallest e with
    amax * 2^-e <= 448), e = 0 for an all-zero row; bytes = float8_e4m3fn(ldexp(x, -e)).  x [..., E] -> (uint8 [..., E], int32 [...])"""
    xf = x.float()
    amax = xf.abs().amax(-1)
    fr, ex = torch.frexp(amax)
    e = torch.where(fr <= 0.875, ex - 9, ex - 8)
    e = torch.where(amax > 0, e, torch.zeros_like(e)).to(torch.int32)
    scaled = torch.ldexp(xf, -e.unsqueeze(-1))
    return scaled.to(torch.float8_e4m3fn).view(torch.uint8), e


def counts_model(txt):
    """`clipx_maxsim_pack_text`'s cnt: the rows up to the last one that differs from the final row, plus one representative"""
    nt, n, _ = txt.shape
    bits = txt.view(torch.int16)
    differs = (bits != bits[:, -1:, :]).any(-1)                                   # [nt, n]
    last = torch.where(differs.any(1), (differs * torch.arange(n)).amax(1), torch.full((nt,), -1))
    return (last + 2).to(torch.int32)
