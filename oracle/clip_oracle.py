"""CPU ORACLE — test infrastructure only, never shipped or measured as product.

A plain-PyTorch (fp32, CPU) restatement of the reference's CLIP train-step hot
path, written as explicit tensor math (no nn.MultiheadAttention, no nn.Conv2d) so
every line can be compared with the HIP kernels.  Only `tests/`,
`__graft_entry__.smoke()` and `bench.py --full`'s `cpu_baseline` leg may import this.

Pinning: the reference ships no tests or golden vectors, so this
restatement is pinned by fixtures generated in the build container by importing
the reference's own `transformer.py` and `loss.py`
(`tests/golden/make_golden.py`; checked by `tests/test_oracle_golden.py`).
The `CLIP` wrapper itself lives in the un-vendored, unpinned third-party package
`open_clip_torch` (reference `src/requirements.txt:3-4`); its arithmetic is
restated from the in-repo mirror `model.py:569-609,656-668`.

Reference lines followed (all under /root/reference/src/colxlip/):
  layer_norm            transformer.py:14-29   (eps 1e-5)
  quick_gelu            transformer.py:32-35
  resblock              transformer.py:213-268 (nn.MultiheadAttention packed in_proj, q|k|v)
  transformer           transformer.py:495-508
  vision_embeds/_pool   transformer.py:701-741, 825-836
  text tower            transformer.py:960-989, 1076-1101, 839-855
  clip forward          model.py:544-556, 569-609, 656-668 (normalize, logit_scale.exp())
  gather_features       loss.py:48-92
  ClipLoss              loss.py:95-182
  AdamW grouping        ../main.py:280-295 ; clamp train.py:211-212
  text init             transformer.py:925-946 ; vision init transformer.py:558-562,624
"""
from __future__ import annotations

import math
from dataclasses import dataclass, asdict
from typing import Dict, List, Optional, Sequence, Tuple

import torch
import torch.nn.functional as F


# --------------------------------------------------------------------------- config
@dataclass
class ClipCfg:
    embed_dim: int = 512
    image_size: int = 224
    patch_size: int = 32
    vision_width: int = 768
    vision_layers: int = 12
    vision_head_width: int = 64          # model.py:30,145
    context_length: int = 77
    vocab_size: int = 49408
    text_width: int = 512
    text_heads: int = 8
    text_layers: int = 12
    mlp_ratio: float = 4.0
    quick_gelu: bool = False

    @property
    def vision_heads(self) -> int:
        return self.vision_width // self.vision_head_width

    @property
    def grid(self) -> int:
        return self.image_size // self.patch_size

    @property
    def vision_tokens(self) -> int:
        return self.grid * self.grid + 1

    @staticmethod
    def from_model_json(cfg: dict, quick_gelu: bool = False) -> "ClipCfg":
        v, t = cfg["vision_cfg"], cfg["text_cfg"]
        return ClipCfg(
            embed_dim=cfg["embed_dim"], image_size=v["image_size"], patch_size=v["patch_size"],
            vision_width=v["width"], vision_layers=v["layers"],
            vision_head_width=v.get("head_width", 64),
            context_length=t["context_length"], vocab_size=t["vocab_size"],
            text_width=t["width"], text_heads=t["heads"], text_layers=t["layers"],
            mlp_ratio=v.get("mlp_ratio", 4.0), quick_gelu=cfg.get("quick_gelu", quick_gelu))


VIT_B_32 = ClipCfg()
VIT_B_16 = ClipCfg(patch_size=16)
TINY = ClipCfg(embed_dim=32, image_size=32, patch_size=16, vision_width=64, vision_layers=2,
               vision_head_width=32, context_length=77, vocab_size=512, text_width=64,
               text_heads=2, text_layers=2)


# --------------------------------------------------------------------------- init
def _block_keys(prefix: str, i: int) -> str:
    return f"{prefix}transformer.resblocks.{i}."


def init_state_dict(cfg: ClipCfg, seed: int = 0) -> Dict[str, torch.Tensor]:
    """Random init with the reference's distributions and its state-dict schema
    (SURVEY §8 a0).  Vision: PyTorch defaults for Conv2d/Linear/MHA, scale*randn
    for class/pos/proj (transformer.py:558-562,624).  Text: transformer.py:925-946."""
    g = torch.Generator().manual_seed(seed)
    sd: Dict[str, torch.Tensor] = {}

    def randn(*shape, std=1.0):
        return torch.randn(*shape, generator=g) * std

    def kaiming_uniform(out_f, in_f, *rest):
        # nn.Linear / nn.Conv2d default: kaiming_uniform_(a=sqrt(5)) -> U(-1/sqrt(fan_in), 1/sqrt(fan_in))
        fan_in = in_f
        for r in rest:
            fan_in *= r
        bound = 1.0 / math.sqrt(fan_in)
        return (torch.rand(out_f, in_f, *rest, generator=g) * 2 - 1) * bound

    def xavier_uniform(out_f, in_f):
        bound = math.sqrt(6.0 / (in_f + out_f))
        return (torch.rand(out_f, in_f, generator=g) * 2 - 1) * bound

    def bias_uniform(out_f, fan_in):
        bound = 1.0 / math.sqrt(fan_in)
        return (torch.rand(out_f, generator=g) * 2 - 1) * bound

    dv, P = cfg.vision_width, cfg.patch_size
    scale = dv ** -0.5
    sd["visual.class_embedding"] = randn(dv, std=scale)
    sd["visual.positional_embedding"] = randn(cfg.vision_tokens, dv, std=scale)
    sd["visual.proj"] = randn(dv, cfg.embed_dim, std=scale)
    sd["visual.conv1.weight"] = kaiming_uniform(dv, 3, P, P)
    sd["visual.ln_pre.weight"] = torch.ones(dv)
    sd["visual.ln_pre.bias"] = torch.zeros(dv)
    mlp_v = int(dv * cfg.mlp_ratio)
    for i in range(cfg.vision_layers):
        p = _block_keys("visual.", i)
        sd[p + "ln_1.weight"] = torch.ones(dv)
        sd[p + "ln_1.bias"] = torch.zeros(dv)
        sd[p + "attn.in_proj_weight"] = xavier_uniform(3 * dv, dv)      # nn.MultiheadAttention default
        sd[p + "attn.in_proj_bias"] = torch.zeros(3 * dv)
        sd[p + "attn.out_proj.weight"] = kaiming_uniform(dv, dv)
        sd[p + "attn.out_proj.bias"] = torch.zeros(dv)
        sd[p + "ln_2.weight"] = torch.ones(dv)
        sd[p + "ln_2.bias"] = torch.zeros(dv)
        sd[p + "mlp.c_fc.weight"] = kaiming_uniform(mlp_v, dv)
        sd[p + "mlp.c_fc.bias"] = bias_uniform(mlp_v, dv)
        sd[p + "mlp.c_proj.weight"] = kaiming_uniform(dv, mlp_v)
        sd[p + "mlp.c_proj.bias"] = bias_uniform(dv, mlp_v)
    sd["visual.ln_post.weight"] = torch.ones(dv)
    sd["visual.ln_post.bias"] = torch.zeros(dv)

    dt = cfg.text_width
    mlp_t = int(dt * cfg.mlp_ratio)
    sd["token_embedding.weight"] = randn(cfg.vocab_size, dt, std=0.02)
    sd["positional_embedding"] = randn(cfg.context_length, dt, std=0.01)
    proj_std = (dt ** -0.5) * ((2 * cfg.text_layers) ** -0.5)
    attn_std = dt ** -0.5
    fc_std = (2 * dt) ** -0.5
    for i in range(cfg.text_layers):
        p = _block_keys("", i)
        sd[p + "ln_1.weight"] = torch.ones(dt)
        sd[p + "ln_1.bias"] = torch.zeros(dt)
        sd[p + "attn.in_proj_weight"] = randn(3 * dt, dt, std=attn_std)
        sd[p + "attn.in_proj_bias"] = torch.zeros(3 * dt)
        sd[p + "attn.out_proj.weight"] = randn(dt, dt, std=proj_std)
        sd[p + "attn.out_proj.bias"] = torch.zeros(dt)
        sd[p + "ln_2.weight"] = torch.ones(dt)
        sd[p + "ln_2.bias"] = torch.zeros(dt)
        sd[p + "mlp.c_fc.weight"] = randn(mlp_t, dt, std=fc_std)
        sd[p + "mlp.c_fc.bias"] = bias_uniform(mlp_t, dt)
        sd[p + "mlp.c_proj.weight"] = randn(dt, mlp_t, std=proj_std)
        sd[p + "mlp.c_proj.bias"] = bias_uniform(dt, mlp_t)
    sd["ln_final.weight"] = torch.ones(dt)
    sd["ln_final.bias"] = torch.zeros(dt)
    sd["text_projection"] = randn(dt, cfg.embed_dim, std=dt ** -0.5)
    sd["logit_scale"] = torch.tensor(math.log(1 / 0.07))                # model.py:470
    return sd


def perturb_state_dict(sd: Dict[str, torch.Tensor], seed: int = 1, amount: float = 0.05):
    """Make LayerNorm gains/biases and zero-initialised biases non-trivial so parity
    tests exercise every parameter (fresh init has gamma=1, beta=0, attn biases=0)."""
    g = torch.Generator().manual_seed(seed)
    out = {}
    for k, v in sd.items():
        if k == "logit_scale":
            out[k] = v.clone()
        elif v.ndim <= 1 and ("ln" in k or "bias" in k):
            out[k] = v + amount * torch.randn(v.shape, generator=g)
        else:
            out[k] = v.clone()
    return out


# --------------------------------------------------------------------------- ops
def layer_norm(x, w, b, eps: float = 1e-5):
    mu = x.mean(dim=-1, keepdim=True)
    xc = x - mu
    var = (xc * xc).mean(dim=-1, keepdim=True)
    return xc * torch.rsqrt(var + eps) * w + b


def quick_gelu(x):
    return x * torch.sigmoid(1.702 * x)


def gelu(x):
    return 0.5 * x * (1.0 + torch.erf(x * (1.0 / math.sqrt(2.0))))


def causal_mask(n: int) -> torch.Tensor:
    m = torch.full((n, n), float("-inf"))
    return torch.triu(m, 1)


def attention(x, in_w, in_b, out_w, out_b, heads: int, mask: Optional[torch.Tensor]):
    """nn.MultiheadAttention(batch_first=True, need_weights=False) self-attention."""
    b, L, d = x.shape
    hd = d // heads
    qkv = x @ in_w.t() + in_b
    q, k, v = qkv.split(d, dim=-1)
    q = q.view(b, L, heads, hd).transpose(1, 2)
    k = k.view(b, L, heads, hd).transpose(1, 2)
    v = v.view(b, L, heads, hd).transpose(1, 2)
    s = (q @ k.transpose(-1, -2)) * (hd ** -0.5)
    if mask is not None:
        s = s + mask
    p = torch.softmax(s, dim=-1)
    o = (p @ v).transpose(1, 2).reshape(b, L, d)
    return o @ out_w.t() + out_b


def resblock(x, sd, p: str, heads: int, mask, act):
    a = layer_norm(x, sd[p + "ln_1.weight"], sd[p + "ln_1.bias"])
    x = x + attention(a, sd[p + "attn.in_proj_weight"], sd[p + "attn.in_proj_bias"],
                      sd[p + "attn.out_proj.weight"], sd[p + "attn.out_proj.bias"], heads, mask)
    c = layer_norm(x, sd[p + "ln_2.weight"], sd[p + "ln_2.bias"])
    u = c @ sd[p + "mlp.c_fc.weight"].t() + sd[p + "mlp.c_fc.bias"]
    x = x + act(u) @ sd[p + "mlp.c_proj.weight"].t() + sd[p + "mlp.c_proj.bias"]
    return x


def patchify(image: torch.Tensor, P: int) -> torch.Tensor:
    """[b,3,H,W] -> [b, G*G, 3*P*P] with inner order (c, py, px) == conv1.weight.view(dv,-1)."""
    b, c, H, W = image.shape
    gh, gw = H // P, W // P
    x = image.reshape(b, c, gh, P, gw, P).permute(0, 2, 4, 1, 3, 5)
    return x.reshape(b, gh * gw, c * P * P)


def vision_forward(sd, image, cfg: ClipCfg, return_tokens: bool = False):
    act = quick_gelu if cfg.quick_gelu else gelu
    dv = cfg.vision_width
    x = patchify(image, cfg.patch_size) @ sd["visual.conv1.weight"].reshape(dv, -1).t()
    cls = sd["visual.class_embedding"].view(1, 1, dv).expand(x.shape[0], 1, dv)
    x = torch.cat([cls, x], dim=1) + sd["visual.positional_embedding"]
    x = layer_norm(x, sd["visual.ln_pre.weight"], sd["visual.ln_pre.bias"])
    for i in range(cfg.vision_layers):
        x = resblock(x, sd, _block_keys("visual.", i), cfg.vision_heads, None, act)
    x = layer_norm(x, sd["visual.ln_post.weight"], sd["visual.ln_post.bias"])
    pooled = x[:, 0] @ sd["visual.proj"]
    return (pooled, x[:, 1:]) if return_tokens else pooled


def text_forward(sd, text, cfg: ClipCfg, return_tokens: bool = False):
    act = quick_gelu if cfg.quick_gelu else gelu
    L = text.shape[1]
    x = sd["token_embedding.weight"][text] + sd["positional_embedding"][:L]
    mask = causal_mask(L)
    for i in range(cfg.text_layers):
        x = resblock(x, sd, _block_keys("", i), cfg.text_heads, mask, act)
    x = layer_norm(x, sd["ln_final.weight"], sd["ln_final.bias"])
    pooled = x[torch.arange(x.shape[0]), text.argmax(dim=-1)] @ sd["text_projection"]
    return (pooled, x) if return_tokens else pooled


def l2_normalize(x, eps: float = 1e-12):
    return x / x.norm(dim=-1, keepdim=True).clamp_min(eps)


def clip_forward(sd, image, text, cfg: ClipCfg):
    return {
        "image_features": l2_normalize(vision_forward(sd, image, cfg)),
        "text_features": l2_normalize(text_forward(sd, text, cfg)),
        "logit_scale": sd["logit_scale"].exp(),
    }


# --------------------------------------------------------------------------- loss
def _ce_arange(logits: torch.Tensor, offset: int = 0) -> torch.Tensor:
    idx = torch.arange(logits.shape[0]) + offset
    return (torch.logsumexp(logits, dim=-1) - logits[torch.arange(logits.shape[0]), idx]).mean()


def clip_loss_single(image_features, text_features, logit_scale):
    """world_size == 1 branch, loss.py:151-152,175-180."""
    li = logit_scale * image_features @ text_features.t()
    lt = logit_scale * text_features @ image_features.t()
    return (_ce_arange(li) + _ce_arange(lt)) / 2


def colbert_similarity(token_image_features, token_text_features):
    """loss.py:20-46: sim[m,k] = mean over the text tokens n of image k's best-matching token, counting only the
    (m,k,n) whose maximum is not exactly 0 (zeroed text tokens).  Explicit loops over the token axes."""
    nt, ni = token_text_features.shape[0], token_image_features.shape[0]
    rows = []
    for m in range(nt):
        row = []
        for k in range(ni):
            s = token_text_features[m] @ token_image_features[k].t()          # [n_txt, n_img]
            best = s.max(dim=1).values
            cnt = (best != 0).float().sum() + 1e-8
            row.append(best.sum() / cnt)
        rows.append(torch.stack(row))
    return torch.stack(rows)


def colclip_loss_single(image_features, text_features, token_image_features, token_text_features, logit_scale, alpha=0.5):
    """ColClipLoss, world_size == 1 (loss.py:259-296): alpha * global CLIP loss + (1 - alpha) * the same symmetric
    cross-entropy on logit_scale * MaxSim token logits."""
    glob = clip_loss_single(image_features, text_features, logit_scale)
    ltt = logit_scale * colbert_similarity(token_image_features, token_text_features)
    tok = (_ce_arange(ltt.t()) + _ce_arange(ltt)) / 2
    return {"global_contrastive_loss": glob, "token_contrastive_loss": tok, "total_loss": alpha * glob + (1 - alpha) * tok}


def clip_loss_rank(img_list: Sequence[torch.Tensor], txt_list: Sequence[torch.Tensor], rank: int,
                   logit_scale, local_loss: bool, gather_with_grad: bool):
    """Loss seen by `rank` when W ranks hold img_list[r], txt_list[r] (loss.py:75-92,132-180).
    Differentiating sum_r clip_loss_rank(..., r) w.r.t. img_list[q] gives exactly what
    reaches rank q's features after the all-gather backward (a reduce-scatter SUM when
    gather_with_grad, nothing from other ranks otherwise)."""
    W = len(img_list)
    if gather_with_grad:
        gi, gt = list(img_list), list(txt_list)
    else:
        gi = [t.detach() for t in img_list]
        gt = [t.detach() for t in txt_list]
        if not local_loss:
            gi[rank], gt[rank] = img_list[rank], txt_list[rank]
    all_i, all_t = torch.cat(gi, 0), torch.cat(gt, 0)
    if local_loss:
        li = logit_scale * img_list[rank] @ all_t.t()
        lt = logit_scale * txt_list[rank] @ all_i.t()
        off = img_list[rank].shape[0] * rank if W > 1 else 0
        return (_ce_arange(li, off) + _ce_arange(lt, off)) / 2
    li = logit_scale * all_i @ all_t.t()
    return (_ce_arange(li) + _ce_arange(li.t())) / 2


def colclip_loss_rank(feats: Sequence[Sequence[torch.Tensor]], rank: int, logit_scale, gather_with_grad: bool, alpha=0.5):
    """ColClipLoss seen by `rank` when W ranks hold feats[r] = (image, text, token_image, token_text) (loss.py:222-262: both
    pairs go through gather_features, logits are global on every rank; local_loss is NotImplemented there).  As for
    clip_loss_rank, differentiating sum_r colclip_loss_rank(..., r) w.r.t. rank q's leaves gives what reaches them."""
    if gather_with_grad:
        cols = [[f[i] for f in feats] for i in range(4)]
    else:
        cols = [[(f[i] if r == rank else f[i].detach()) for r, f in enumerate(feats)] for i in range(4)]
    fi, ft, ti, tt = (torch.cat(c, 0) for c in cols)
    return colclip_loss_single(fi, ft, ti, tt, logit_scale, alpha)


def colclip_loss_rank_rows_local(feats: Sequence[Sequence[torch.Tensor]], rank: int, logit_scale, alpha=0.5):
    """`ColClipLoss(rows_local=True, gather_with_grad=True)` (an extension of the build; the reference computes the global logits
    on every rank): the loss rank `rank` returns when it owns only ITS text rows of the token logits and ClipLoss's local-loss
    convention (loss.py:119-130,144-146) is applied to both terms.  A plain function of ALL ranks' leaves, so that
    differentiating sum_r colclip_loss_rank_rows_local(..., r) gives what the collectives deliver; its mean over ranks is
    colclip_loss_single on the concatenated features."""
    fi, ft, ti, tt = (torch.cat([f[i] for f in feats], 0) for i in range(4))
    b = feats[rank][0].shape[0]
    off = b * rank
    mine = slice(off, off + b)
    glob = (_ce_arange(logit_scale * fi[mine] @ ft.t(), off) + _ce_arange(logit_scale * ft[mine] @ fi.t(), off)) / 2
    z = logit_scale * colbert_similarity(ti, tt)                    # [N text, N image]
    rows = _ce_arange(z[mine], off)                                   # mean over this rank's text rows
    cols = (torch.logsumexp(z, dim=0)[mine] - z[mine][torch.arange(b), off + torch.arange(b)]).mean()     # its images' columns
    tok = (rows + cols) / 2
    return {"global_contrastive_loss": glob, "token_contrastive_loss": tok, "total_loss": alpha * glob + (1 - alpha) * tok}


# --------------------------------------------------------------------------- optimizer
def adamw_exclude(name: str, p: torch.Tensor) -> bool:
    """main.py:280 — weight-decay-free group."""
    return p.ndim < 2 or "bn" in name or "ln" in name or "bias" in name or "logit_scale" in name


def adamw_step(params: Dict[str, torch.Tensor], grads: Dict[str, torch.Tensor],
               m: Dict[str, torch.Tensor], v: Dict[str, torch.Tensor], step: int,
               lr: float = 5e-4, beta1: float = 0.9, beta2: float = 0.98, eps: float = 1e-6,
               wd: float = 0.2):
    """torch.optim.AdamW (decoupled wd) with the reference's two groups, in place;
    then logit_scale.clamp_(0, ln 100) (train.py:211-212).  `step` is 1-based."""
    bc1 = 1.0 - beta1 ** step
    bc2 = 1.0 - beta2 ** step
    for k, p in params.items():
        g = grads[k]
        decay = 0.0 if adamw_exclude(k, p) else wd
        p.mul_(1.0 - lr * decay)
        m[k].mul_(beta1).add_(g, alpha=1.0 - beta1)
        v[k].mul_(beta2).addcmul_(g, g, value=1.0 - beta2)
        denom = (v[k].sqrt() / math.sqrt(bc2)).add_(eps)
        p.addcdiv_(m[k], denom, value=-lr / bc1)
    params["logit_scale"].clamp_(0, math.log(100))


# --------------------------------------------------------------------------- synthetic data
def synthetic_batch(cfg: ClipCfg, batch: int, seed: int = 1234):
    """images ~ N(0,1); token ids U[1, vocab-2), one EOT (= vocab-1, the max id)
    at a random position in [8, L-1], zeros after it."""
    g = torch.Generator().manual_seed(seed)
    images = torch.randn(batch, 3, cfg.image_size, cfg.image_size, generator=g)
    L = cfg.context_length
    text = torch.randint(1, cfg.vocab_size - 2, (batch, L), generator=g)
    eot = torch.randint(8, L, (batch,), generator=g)
    pos = torch.arange(L).unsqueeze(0)
    text = torch.where(pos < eot.unsqueeze(1), text, torch.zeros_like(text))
    text[torch.arange(batch), eot] = cfg.vocab_size - 1
    return images, text


# --------------------------------------------------------------------------- train step
def loss_and_grads(sd: Dict[str, torch.Tensor], image, text, cfg: ClipCfg):
    """Single-rank forward + backward; returns (out dict, loss, grads by state-dict key)."""
    leaves = {k: v.detach().clone().requires_grad_(True) for k, v in sd.items()}
    out = clip_forward(leaves, image, text, cfg)
    loss = clip_loss_single(out["image_features"], out["text_features"], out["logit_scale"])
    loss.backward()
    grads = {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in leaves.items()}
    return {k: v.detach() for k, v in out.items()}, loss.detach(), grads


def train_steps(sd: Dict[str, torch.Tensor], batches, cfg: ClipCfg, **opt):
    """In-place multi-step training on copies; returns (final params, losses)."""
    params = {k: v.detach().clone() for k, v in sd.items()}
    m = {k: torch.zeros_like(v) for k, v in params.items()}
    v_ = {k: torch.zeros_like(v) for k, v in params.items()}
    losses = []
    for step, (image, text) in enumerate(batches, 1):
        _, loss, grads = loss_and_grads(params, image, text, cfg)
        losses.append(float(loss))
        adamw_step(params, grads, m, v_, step, **opt)
    return params, losses


# --------------------------------------------------------------------------- ColXLIP ("next" row)
def init_colxlip_heads(cfg: ClipCfg, seed: int = 0) -> Dict[str, torch.Tensor]:
    """Token projection heads nn.Sequential(LayerNorm, Linear, GELU, LayerNorm) with PyTorch default init
    (reference model.py:514-526); keys as in the reference's state dict."""
    g = torch.Generator().manual_seed(seed + 1000)
    sd: Dict[str, torch.Tensor] = {}
    for name, width in (("vision_token_layer", cfg.vision_width), ("text_token_layer", cfg.text_width)):
        bound = 1.0 / math.sqrt(width)
        sd[f"{name}.0.weight"] = torch.ones(width)
        sd[f"{name}.0.bias"] = torch.zeros(width)
        sd[f"{name}.1.weight"] = (torch.rand(cfg.embed_dim, width, generator=g) * 2 - 1) * bound
        sd[f"{name}.1.bias"] = (torch.rand(cfg.embed_dim, generator=g) * 2 - 1) * bound
        sd[f"{name}.3.weight"] = torch.ones(cfg.embed_dim)
        sd[f"{name}.3.bias"] = torch.zeros(cfg.embed_dim)
    return sd


def colxlip_state_dict(cfg: ClipCfg, head_seed: int = 5) -> Dict[str, torch.Tensor]:
    """Seeded ColXLIP weights of the `colxlip_*` fixtures (tests/golden/make_golden.py:golden_colxlip): the CLIP state
    dict of the other fixtures + the two token heads, every LayerNorm gain of the heads moved off 1 as well
    (perturb_state_dict moves only biases and `ln*` keys)."""
    sd = perturb_state_dict(init_state_dict(cfg, seed=0), seed=1)
    heads = perturb_state_dict(init_colxlip_heads(cfg, seed=head_seed), seed=head_seed + 1)
    g = torch.Generator().manual_seed(head_seed + 2)
    for k in heads:
        if k.endswith((".0.weight", ".3.weight")):
            heads[k] = heads[k] + 0.05 * torch.randn(heads[k].shape, generator=g)
    sd.update(heads)
    return sd


def token_head(x, sd, name: str):
    x = layer_norm(x, sd[f"{name}.0.weight"], sd[f"{name}.0.bias"])
    x = gelu(x @ sd[f"{name}.1.weight"].t() + sd[f"{name}.1.bias"])
    return layer_norm(x, sd[f"{name}.3.weight"], sd[f"{name}.3.bias"])


def colxlip_forward(sd, image, text, cfg: ClipCfg):
    """reference model.py:529-603,643-668: global features as CLIP; image tokens = ln_post'd patch tokens through the
    vision head; text tokens = ln_final'd tokens with every position at or after the EOT (arg-max id) zeroed BEFORE the
    text head; everything L2-normalised."""
    pooled_i, tok_i = vision_forward(sd, image, cfg, return_tokens=True)
    pooled_t, tok_t = text_forward(sd, text, cfg, return_tokens=True)
    L = text.shape[1]
    keep = (torch.arange(L).unsqueeze(0) < text.argmax(dim=-1).unsqueeze(1)).unsqueeze(-1)
    tok_t = torch.where(keep, tok_t, torch.zeros_like(tok_t))
    return {
        "image_features": l2_normalize(pooled_i),
        "text_features": l2_normalize(pooled_t),
        "token_image_features": l2_normalize(token_head(tok_i, sd, "vision_token_layer")),
        "token_text_features": l2_normalize(token_head(tok_t, sd, "text_token_layer")),
        "logit_scale": sd["logit_scale"].exp(),
    }


def colxlip_loss_and_grads(sd: Dict[str, torch.Tensor], image, text, cfg: ClipCfg, alpha: float = 0.5):
    leaves = {k: v.detach().clone().requires_grad_(True) for k, v in sd.items()}
    out = colxlip_forward(leaves, image, text, cfg)
    res = colclip_loss_single(out["image_features"], out["text_features"], out["token_image_features"],
                              out["token_text_features"], out["logit_scale"], alpha)
    res["total_loss"].backward()
    grads = {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in leaves.items()}
    return {k: v.detach() for k, v in out.items()}, {k: v.detach() for k, v in res.items()}, grads


# --------------------------------------------------------------------------- retrieval evaluation
def retrieval_metrics(similarity: torch.Tensor, txt2img, img2txt) -> Dict[str, float]:
    """Reference train.py:457-508 restated: `similarity` [n_img, n_txt]; txt2img[c] = image row of caption c; img2txt[i] = caption
    rows of image i.  Rank of the true item in the descending argsort of every row; for an image the best rank over its
    captions.  R@k = share of ranks < k; mean rank from a float32 vector (+1); median = floor(median)+1."""
    import numpy as np
    t2i = similarity.t()
    t_ranks = torch.zeros(t2i.shape[0])
    for c, row in enumerate(t2i):
        order = torch.argsort(row, descending=True)
        t_ranks[c] = torch.where(order == txt2img[c])[0][0]
    i_ranks = torch.zeros(similarity.shape[0])
    for i, row in enumerate(similarity):
        order = torch.argsort(row, descending=True)
        i_ranks[i] = min(int(torch.where(order == c)[0][0]) for c in img2txt[i])

    def report(prefix, ranks):
        n = len(ranks)
        return {f"{prefix}_R@1": float((ranks < 1).sum()) / n, f"{prefix}_R@5": float((ranks < 5).sum()) / n,
                f"{prefix}_R@10": float((ranks < 10).sum()) / n, f"{prefix}_mean_rank": ranks.mean().item() + 1,
                f"{prefix}_median_rank": float(np.floor(np.median(ranks.numpy())) + 1)}

    return {**report("text_to_image", t_ranks), **report("image_to_text", i_ranks)}


def retrieval_eval(sd, images, img_ids, texts, img2txt_dict, txt2img_dict, cfg: ClipCfg) -> Dict[str, float]:
    """Reference train.py:510-608 (`original_clip` mode) on the oracle towers: encode both sides, logit_scale * I @ T^T,
    dataset image ids -> rows (train.py:429-454), metrics."""
    with torch.no_grad():
        fi = l2_normalize(vision_forward(sd, images, cfg))
        ft = l2_normalize(text_forward(sd, texts, cfg))
        sim = sd["logit_scale"].exp() * fi @ ft.t()
    row_of = {int(old): row for row, old in enumerate(img_ids.tolist())}
    img2txt = {row_of[i]: list(caps) for i, caps in img2txt_dict.items()}
    txt2img = {c: row_of[imgs[0]] for c, imgs in txt2img_dict.items()}
    return retrieval_metrics(sim, txt2img, img2txt)


# --------------------------------------------------------------------------- gradient sketches (test infrastructure)
def count_sketch(g: torch.Tensor, buckets: int = 128, chunk: int = 1 << 22) -> torch.Tensor:
    """CountSketch of a tensor: element i goes to bucket h(i) with sign s(i), both from an integer hash of the flat index
    computed with wrapping int64 arithmetic (identical on CPU and GPU, no random-number generator involved):
        sketch[b] = sum_{i: h(i) = b} s(i) * g[i]                       (float64 accumulation)
    Inner products -- hence the COSINE between two gradients of the same parameter -- are preserved in expectation with a
    variance that vanishes as the two vectors align, and every element contributes with equal weight whatever its position:
    unlike a strided sample or sums of contiguous blocks it is not at the mercy of one row that is 300x larger than the
    others (visual.positional_embedding: class-token row vs patch rows).  `buckets` must be a power of two."""
    flat = g.reshape(-1)
    out = torch.zeros(buckets, dtype=torch.float64, device=flat.device)
    for lo in range(0, flat.numel(), chunk):
        part = flat[lo:lo + chunk].double()
        x = torch.arange(lo, lo + part.numel(), dtype=torch.int64, device=flat.device)
        x = x * -7046029254386353131                      # 0x9E3779B97F4A7C15 as a signed 64-bit integer (wraps)
        x = x ^ ((x >> 29) & 0x7FFFFFFFF)
        x = x * -4658895280553007687                      # 0xBF58476D1CE4E5B9
        x = x ^ ((x >> 32) & 0xFFFFFFFF)
        bucket = (x >> 40) & (buckets - 1)
        sign = (((x >> 20) & 1) * 2 - 1).double()
        # (bincount, not index_add_: 4 M fp64 atomic adds onto 128 addresses took ~0.4 s per chunk on the GPU)
        out += torch.bincount(bucket, weights=part * sign, minlength=buckets)
    return out
