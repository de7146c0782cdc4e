"""Generate golden fixtures by IMPORTING the reference's own files.

Runs only in the build container (needs /root/reference; the GPU box has no
reference).  Imports `src/colxlip/transformer.py` and `src/colxlip/loss.py`
exactly as SURVEY.md §8c describes (torchvision.ops.misc stubbed: it is needed by
utils.py:8 only and never by this path), runs them on seeded inputs and writes
small .npz files of inputs + expected outputs next to this script.  The fixtures
are data only; no reference source text is stored.

    python tests/golden/make_golden.py            # all fixtures
"""
import importlib
import importlib.util
import math
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
REF = "/root/reference/src/colxlip"

from oracle import clip_oracle as O  # noqa: E402


def import_reference():
    tv = types.ModuleType("torchvision")
    ops = types.ModuleType("torchvision.ops")
    misc = types.ModuleType("torchvision.ops.misc")

    class FrozenBatchNorm2d(torch.nn.Module):
        pass

    misc.FrozenBatchNorm2d = FrozenBatchNorm2d
    sys.modules.update({"torchvision": tv, "torchvision.ops": ops, "torchvision.ops.misc": misc})
    pkg = types.ModuleType("refcolxlip")
    pkg.__path__ = [REF]
    sys.modules["refcolxlip"] = pkg
    T = importlib.import_module("refcolxlip.transformer")
    spec = importlib.util.spec_from_file_location("ref_loss", REF + "/loss.py")
    L = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(L)
    return T, L


def build_ref_towers(T, cfg: O.ClipCfg, sd):
    act = T.QuickGELU if cfg.quick_gelu else torch.nn.GELU
    vis = T.VisionTransformer(
        image_size=cfg.image_size, patch_size=cfg.patch_size, width=cfg.vision_width,
        layers=cfg.vision_layers, heads=cfg.vision_heads, mlp_ratio=cfg.mlp_ratio,
        output_dim=cfg.embed_dim, act_layer=act)
    txt = T.TextTransformer(
        context_length=cfg.context_length, vocab_size=cfg.vocab_size, width=cfg.text_width,
        heads=cfg.text_heads, layers=cfg.text_layers, mlp_ratio=cfg.mlp_ratio,
        output_dim=cfg.embed_dim, act_layer=act)
    vis.load_state_dict({k[len("visual."):]: v for k, v in sd.items() if k.startswith("visual.")})
    txt.load_state_dict({k: v for k, v in sd.items() if not k.startswith("visual.") and k != "logit_scale"})
    vis.train()
    txt.train()
    return vis, txt


def ref_clip_step(T, L, cfg, sd, image, text):
    """CLIP.forward arithmetic (mirror model.py:552,606,664) on the reference towers + ClipLoss."""
    vis, txt = build_ref_towers(T, cfg, sd)
    logit_scale = torch.nn.Parameter(sd["logit_scale"].clone())
    img_pooled = vis(image)
    txt_pooled = txt(text)
    img_f = F.normalize(img_pooled, dim=-1)
    txt_f = F.normalize(txt_pooled, dim=-1)
    loss = L.ClipLoss()(img_f, txt_f, logit_scale.exp())
    loss.backward()
    grads = {"visual." + k: p.grad for k, p in vis.named_parameters()}
    grads.update({k: p.grad for k, p in txt.named_parameters()})
    grads["logit_scale"] = logit_scale.grad
    return img_pooled.detach(), txt_pooled.detach(), img_f.detach(), txt_f.detach(), loss.detach(), grads


def save(name, **arrs):
    out = {}
    for k, v in arrs.items():
        if isinstance(v, torch.Tensor):
            v = v.detach().cpu().numpy()
        out[k] = v
    path = os.path.join(HERE, name)
    np.savez_compressed(path, **out)
    print(f"wrote {name}: {os.path.getsize(path) / 1024:.1f} KiB")


def golden_tiny_clip(T, L):
    cfg = O.TINY
    sd = O.perturb_state_dict(O.init_state_dict(cfg, seed=0), seed=1)
    image, text = O.synthetic_batch(cfg, 8, seed=1234)
    ip, tp, fi, ft, loss, grads = ref_clip_step(T, L, cfg, sd, image, text)
    arrs = {"image": image, "text": text, "image_pooled": ip, "text_pooled": tp,
            "image_features": fi, "text_features": ft, "loss": loss}
    for k, v in sd.items():
        arrs["sd/" + k] = v
    for k, v in grads.items():
        arrs["grad/" + k] = v
    save("tiny_clip.npz", **arrs)
    # quick-gelu variant: outputs only
    cfg_q = O.ClipCfg(**{**O.asdict(cfg), "quick_gelu": True})
    ip, tp, fi, ft, loss, grads = ref_clip_step(T, L, cfg_q, sd, image, text)
    save("tiny_clip_quickgelu.npz", image_pooled=ip, text_pooled=tp, loss=loss,
         **{"grad/" + k: grads[k] for k in ("visual.conv1.weight", "token_embedding.weight", "logit_scale")})


REAL_SIZE = {
    # BASELINE.json configs 3-5 at full width/depth, batch 2 (dims: SURVEY section 8; B/16 from the reference's
    # model_configs/ViT-B-16.json, L/14-336 and H/14 are upstream open_clip's)
    "b32": ("ViT-B-32", 4),
    "b16": ("ViT-B-16", 2),
    "l14_336": ("ViT-L-14-336", 2),
    "h14": ("ViT-H-14", 2),
    # round 3: batches at which bias / LayerNorm gradients are not remainders of two cancelling samples, and a strided
    # SAMPLE of every gradient (direction, not only norm)
    "b32x16": ("ViT-B-32", 16),
    "b16x8": ("ViT-B-16", 8),
    "l14_336x4": ("ViT-L-14-336", 4),
    "h14x8": ("ViT-H-14", 8),
}
GRAD_SAMPLE = 128


def grad_sample_index(numel, n=GRAD_SAMPLE):
    """Evenly strided element indices of a flattened gradient (all of it when it has <= n elements); the consumer
    recomputes them from the parameter's size."""
    if numel <= n:
        return torch.arange(numel)
    return (torch.arange(n, dtype=torch.int64) * numel) // n


def real_size_cfg(model_name):
    import json
    with open(os.path.join(ROOT, "colxlip_amd", "model_configs", model_name + ".json")) as f:
        return O.ClipCfg.from_model_json(json.load(f))


def golden_real_size(T, L, tag):
    """Full-size towers of the other BASELINE configs, batch 2, through the reference's own transformer.py /
    loss.py.  Weights are regenerated from the seed by the consumer (checksummed); outputs + gradient summaries only."""
    model_name, batch = REAL_SIZE[tag]
    cfg = real_size_cfg(model_name)
    sd = O.perturb_state_dict(O.init_state_dict(cfg, seed=0), seed=1)
    image, text = O.synthetic_batch(cfg, batch, seed=1234)
    ip, tp, fi, ft, loss, grads = ref_clip_step(T, L, cfg, sd, image, text)
    arrs = {"image_pooled": ip, "text_pooled": tp, "image_features": fi, "text_features": ft,
            "loss": loss, "logits": (sd["logit_scale"].exp() * fi @ ft.t())}
    names = sorted(grads.keys())
    arrs["grad_names"] = np.array(names)
    arrs["grad_norms"] = np.array([float(grads[k].double().norm()) for k in names])
    arrs["grad_head"] = np.stack([
        F.pad(grads[k].reshape(-1)[:8], (0, max(0, 8 - grads[k].numel()))).numpy() for k in names])
    arrs["grad_sample"] = np.stack([
        F.pad(grads[k].reshape(-1)[grad_sample_index(grads[k].numel())], (0, max(0, GRAD_SAMPLE - grads[k].numel()))).numpy()
        for k in names])
    # CountSketch of every gradient (oracle.count_sketch: 128 buckets, hashed bucket + sign per element): the statistic the
    # bf16 direction check uses.  (A strided sample, or sums of contiguous blocks, of a tensor whose rows differ in scale by
    # 300x -- visual.positional_embedding: class-token row vs patch rows -- is decided by whichever entries sit in the large row.)
    arrs["grad_sketch"] = np.stack([O.count_sketch(grads[k]).numpy() for k in names])
    arrs["sd_checksum"] = np.array([float(sd[k].double().sum()) for k in sorted(sd.keys())])
    arrs["n_params"] = np.array(sum(v.numel() for v in sd.values()))
    save(f"{tag.split('x')[0]}_batch{batch}.npz", **arrs)


def golden_loss_w1(L):
    g = torch.Generator().manual_seed(7)
    out = {}
    for tag, n, e in (("a", 16, 32), ("b", 50, 64)):
        fi = F.normalize(torch.randn(n, e, generator=g), dim=-1).requires_grad_(True)
        ft = F.normalize(torch.randn(n, e, generator=g), dim=-1).requires_grad_(True)
        ls = torch.tensor(math.log(1 / 0.07) + 0.3).requires_grad_(True)
        loss_mod = L.ClipLoss()
        li, lt = loss_mod.get_logits(fi, ft, ls.exp())
        loss = loss_mod(fi, ft, ls.exp())
        loss.backward()
        out.update({f"{tag}/image_features": fi, f"{tag}/text_features": ft, f"{tag}/log_logit_scale": ls,
                    f"{tag}/logits_per_image": li, f"{tag}/logits_per_text": lt, f"{tag}/loss": loss,
                    f"{tag}/grad_image": fi.grad, f"{tag}/grad_text": ft.grad, f"{tag}/grad_log_logit_scale": ls.grad})
    save("loss_w1.npz", **out)


def golden_colclip_loss(L):
    """ColClipLoss (reference loss.py:184-296), single rank: global + token (MaxSim) contrastive loss and every gradient."""
    g = torch.Generator().manual_seed(11)
    out = {}
    for tag, n, nt, nq, e in (("a", 6, 5, 7, 16), ("b", 12, 77, 49, 64)):
        fi = F.normalize(torch.randn(n, e, generator=g), dim=-1).requires_grad_(True)
        ft = F.normalize(torch.randn(n, e, generator=g), dim=-1).requires_grad_(True)
        ti = F.normalize(torch.randn(n, nq, e, generator=g), dim=-1).requires_grad_(True)
        tt_raw = F.normalize(torch.randn(n, nt, e, generator=g), dim=-1)
        keep = torch.ones(n, nt, 1)
        for r in range(n):                      # exact-zero token rows: the masked-mean path (loss.py:36-43)
            keep[r, (r % (nt - 1)) + 1:] = 0.0 if r % 3 == 0 else 1.0
        tt = (tt_raw * keep).requires_grad_(True)
        ls = torch.tensor(math.log(1 / 0.07) - 0.5).requires_grad_(True)
        for alpha in (0.5, 0.2):
            for t in (fi, ft, ti, tt, ls):
                t.grad = None
            mod = L.ColClipLoss(alpha=alpha)
            res = mod(image_features=fi, text_features=ft, token_image_features=ti, token_text_features=tt,
                      logit_scale=ls.exp(), output_dict=True)
            res["total_loss"].backward()
            k = f"{tag}/alpha{alpha}"
            out.update({f"{k}/global_loss": res["global_contrastive_loss"], f"{k}/token_loss": res["token_contrastive_loss"],
                        f"{k}/total_loss": res["total_loss"], f"{k}/grad_image": fi.grad.clone(),
                        f"{k}/grad_text": ft.grad.clone(), f"{k}/grad_token_image": ti.grad.clone(),
                        f"{k}/grad_token_text": tt.grad.clone(), f"{k}/grad_log_logit_scale": ls.grad.clone()})
        logits = L.ColClipLoss().get_logits(fi, ft, ti, tt, ls.exp())
        out.update({f"{tag}/image_features": fi, f"{tag}/text_features": ft, f"{tag}/token_image_features": ti,
                    f"{tag}/token_text_features": tt, f"{tag}/log_logit_scale": ls,
                    f"{tag}/logits_per_text_token": logits["logits_per_text_token"]})
    save("colclip_loss.npz", **out)


def _dist_worker(rank, world, port, b, e, q):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    _, L = import_reference()
    g = torch.Generator().manual_seed(100 + rank)
    res = {}
    for local_loss in (False, True):
        for gwg in (False, True):
            fi = F.normalize(torch.randn(b, e, generator=g), dim=-1).requires_grad_(True)
            ft = F.normalize(torch.randn(b, e, generator=g), dim=-1).requires_grad_(True)
            ls = torch.tensor(2.5).requires_grad_(True)
            mod = L.ClipLoss(local_loss=local_loss, gather_with_grad=gwg, cache_labels=True,
                             rank=rank, world_size=world)
            ai, at = L.gather_features(fi, ft, local_loss, gwg, rank, world)
            loss = mod(fi, ft, ls.exp())
            loss.backward()
            tag = f"w{world}/ll{int(local_loss)}_gwg{int(gwg)}/r{rank}"
            res.update({f"{tag}/image_features": fi.detach(), f"{tag}/text_features": ft.detach(),
                        f"{tag}/all_image": ai.detach(), f"{tag}/all_text": at.detach(),
                        f"{tag}/loss": loss.detach(), f"{tag}/grad_image": fi.grad, f"{tag}/grad_text": ft.grad,
                        f"{tag}/grad_log_logit_scale": ls.grad})
    q.put({k: v.numpy() for k, v in res.items()})
    dist.barrier()
    dist.destroy_process_group()


def _colclip_dist_worker(rank, world, port, q):
    """The reference's ColClipLoss over a real gloo group (loss.py:222-262: feature AND token gathers, global logits on
    every rank; local_loss raises NotImplementedError there)."""
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    _, L = import_reference()
    g = torch.Generator().manual_seed(300 + rank)
    b, nt, nq, e = 5, 9, 7, 16
    res = {}
    for gwg in (False, True):
        fi = F.normalize(torch.randn(b, e, generator=g), dim=-1).requires_grad_(True)
        ft = F.normalize(torch.randn(b, e, generator=g), dim=-1).requires_grad_(True)
        ti = F.normalize(torch.randn(b, nq, e, generator=g), dim=-1).requires_grad_(True)
        tt_raw = F.normalize(torch.randn(b, nt, e, generator=g), dim=-1)
        keep = torch.ones(b, nt, 1)
        for r in range(b):                      # exact-zero token rows behind a per-sample length (masked mean, loss.py:36-43)
            keep[r, 2 + (r + rank) % (nt - 2):] = 0.0
        tt = (tt_raw * keep).requires_grad_(True)
        ls = torch.tensor(2.2).requires_grad_(True)
        mod = L.ColClipLoss(local_loss=False, gather_with_grad=gwg, cache_labels=True, rank=rank, world_size=world, alpha=0.3)
        out = mod(image_features=fi, text_features=ft, token_image_features=ti, token_text_features=tt, logit_scale=ls.exp(),
                  output_dict=True)
        out["total_loss"].backward()
        tag = f"w{world}/gwg{int(gwg)}/r{rank}"
        res.update({f"{tag}/image_features": fi.detach(), f"{tag}/text_features": ft.detach(),
                    f"{tag}/token_image_features": ti.detach(), f"{tag}/token_text_features": tt.detach(),
                    f"{tag}/global_loss": out["global_contrastive_loss"].detach(),
                    f"{tag}/token_loss": out["token_contrastive_loss"].detach(), f"{tag}/total_loss": out["total_loss"].detach(),
                    f"{tag}/grad_image": fi.grad, f"{tag}/grad_text": ft.grad, f"{tag}/grad_token_image": ti.grad,
                    f"{tag}/grad_token_text": tt.grad, f"{tag}/grad_log_logit_scale": ls.grad})
    try:
        L.ColClipLoss(local_loss=True, rank=rank, world_size=world)(image_features=fi, text_features=ft, token_image_features=ti,
                                                                    token_text_features=tt, logit_scale=ls.exp())
        res[f"w{world}/local_loss_raises/r{rank}"] = torch.tensor(0)
    except NotImplementedError:
        res[f"w{world}/local_loss_raises/r{rank}"] = torch.tensor(1)
    q.put({k: v.numpy() for k, v in res.items()})
    dist.barrier()
    dist.destroy_process_group()


def golden_colclip_dist():
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    allres = {"alpha": np.array(0.3), "log_logit_scale": np.array(2.2)}
    for world, port in ((2, 29621),):
        q = ctx.Queue()
        procs = [ctx.Process(target=_colclip_dist_worker, args=(r, world, port, q)) for r in range(world)]
        for p in procs:
            p.start()
        for _ in range(world):
            allres.update(q.get())
        for p in procs:
            p.join()
    save("colclip_dist.npz", **allres)


def golden_loss_dist():
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    allres = {}
    for world, port in ((2, 29611), (4, 29612)):
        q = ctx.Queue()
        procs = [ctx.Process(target=_dist_worker, args=(r, world, port, 6, 16, q)) for r in range(world)]
        for p in procs:
            p.start()
        for _ in range(world):
            allres.update(q.get())
        for p in procs:
            p.join()
    save("loss_dist.npz", **allres)


def golden_misc(T, L):
    g = torch.Generator().manual_seed(11)
    out = {}
    # (3) ResidualAttentionBlock with / without causal mask, fwd + all grads
    d, h, Lq, b = 64, 2, 13, 3
    blk = T.ResidualAttentionBlock(d, h)
    blk.train()
    with torch.no_grad():
        for p in blk.parameters():
            p.add_(0.05 * torch.randn(p.shape, generator=g))
    for k, v in blk.state_dict().items():
        out["block/sd/" + k] = v.clone()
    x = torch.randn(b, Lq, d, generator=g)
    out["block/x"] = x
    for tag, mask in (("nomask", None), ("causal", torch.triu(torch.full((Lq, Lq), float("-inf")), 1))):
        blk.zero_grad()
        xi = x.clone().requires_grad_(True)
        y = blk(xi, attn_mask=mask)
        w = torch.randn(y.shape, generator=torch.Generator().manual_seed(5))
        (y * w).sum().backward()
        out[f"block/{tag}/y"] = y.detach()
        out[f"block/{tag}/dy"] = w
        out[f"block/{tag}/dx"] = xi.grad
        for k, p in blk.named_parameters():
            out[f"block/{tag}/grad/{k}"] = p.grad.clone()
    # (5) LayerNormFp32 on bf16 input
    ln = T.LayerNormFp32(96)
    with torch.no_grad():
        ln.weight.add_(0.1 * torch.randn(96, generator=g))
        ln.bias.add_(0.1 * torch.randn(96, generator=g))
    xb = torch.randn(10, 96, generator=g).to(torch.bfloat16)
    out["lnfp32/x_bf16_as_f32"] = xb.float()
    out["lnfp32/w"] = ln.weight.detach()
    out["lnfp32/b"] = ln.bias.detach()
    out["lnfp32/y_bf16_as_f32"] = ln(xb).float()
    # (6) text_global_pool argmax
    xt = torch.randn(5, 9, 4, generator=g)
    tt = torch.randint(0, 50, (5, 9), generator=g)
    out["pool/x"] = xt
    out["pool/text"] = tt
    out["pool/pooled"] = T.text_global_pool(xt, tt, "argmax")
    # (7) init statistics of TextTransformer.init_parameters
    txt = T.TextTransformer(context_length=77, vocab_size=2048, width=128, heads=2, layers=3, output_dim=64)
    names, stds = [], []
    for k, p in txt.named_parameters():
        if p.ndim >= 2:
            names.append(k)
            stds.append(float(p.std()))
    out["textinit/names"] = np.array(names)
    out["textinit/stds"] = np.array(stds)
    out["textinit/causal_mask"] = txt.attn_mask
    # (8) compute_colbert_similarity ("next" row)
    ti = F.normalize(torch.randn(4, 7, 16, generator=g), dim=-1)
    tx = F.normalize(torch.randn(5, 6, 16, generator=g), dim=-1)
    tx[1, 4:] = 0
    out["colbert/token_image"] = ti
    out["colbert/token_text"] = tx
    out["colbert/sim"] = L.compute_colbert_similarity(ti, tx)
    save("misc.npz", **out)


def golden_lp(T):
    """the reference's own `convert_weights_to_lp` (model.py:228-255) run on the reference's towers.  model.py itself
    cannot be imported (it imports open_clip at module level), so that one function is taken out of its source with `ast` and
    executed with the names it refers to bound to the reference's transformer.py classes (`CLIP` = open_clip's class, of which
    no instance exists here, is bound to a placeholder type).  Stored: which parameters changed dtype, and every tensor's
    value afterwards (as fp32) for the TINY config with the oracle's seeded weights."""
    import ast
    src = open(REF + "/model.py").read()
    fn = next(n for n in ast.parse(src).body if isinstance(n, ast.FunctionDef) and n.name == "convert_weights_to_lp")
    ns = {"torch": torch, "nn": torch.nn, "Attention": T.Attention, "TextTransformer": T.TextTransformer,
          "VisionTransformer": T.VisionTransformer, "CLIP": type("CLIP", (), {})}
    exec(compile(ast.Module(body=[fn], type_ignores=[]), REF + "/model.py", "exec"), ns)
    cfg = O.TINY
    sd = O.perturb_state_dict(O.init_state_dict(cfg, seed=0), seed=1)
    vis, txt = build_ref_towers(T, cfg, sd)
    ns["convert_weights_to_lp"](vis, dtype=torch.bfloat16)
    ns["convert_weights_to_lp"](txt, dtype=torch.bfloat16)
    after = {"visual." + k: v for k, v in vis.state_dict().items()}
    after.update({k: v for k, v in txt.state_dict().items() if k != "attn_mask"})
    cast = sorted(k for k, v in after.items() if v.dtype == torch.bfloat16)
    arrs = {"cast_names": np.array(cast), "all_names": np.array(sorted(after))}
    for k, v in after.items():
        arrs["after/" + k] = v.float()
    save("lp_convert.npz", **arrs)


def golden_checkpoint(T):
    """the reference's own checkpoint-interop functions -- `resize_pos_embed`, `resize_text_pos_embed`,
    `convert_to_custom_text_state_dict` (model.py:262-277,355-418) and `load_state_dict` (factory.py:144-156) -- taken out of
    their sources with `ast` (model.py / factory.py import open_clip at module level) and executed as they stand.  The `model`
    they inspect is the reference's own VisionTransformer (grid_size) plus a positional_embedding of the target length.
    Stored: inputs, outputs, and -- for load_state_dict -- what it returns for the three file layouts (bare state dict, train
    checkpoint, DistributedDataParallel-saved `module.` keys)."""
    import ast
    import logging
    import tempfile
    from itertools import repeat
    import collections.abc

    def take(path, names):
        tree = ast.parse(open(path).read())
        return [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in names]

    def _ntuple(n):            # open_clip.utils.to_2tuple (third party; two lines of plain Python)
        def parse(x):
            return tuple(x) if isinstance(x, collections.abc.Iterable) else tuple(repeat(x, n))
        return parse

    ns = {"torch": torch, "F": F, "math": math, "logging": logging, "to_2tuple": _ntuple(2)}
    exec(compile(ast.Module(body=take(REF + "/model.py", ("resize_pos_embed", "resize_text_pos_embed",
                                                          "convert_to_custom_text_state_dict")), type_ignores=[]),
                 REF + "/model.py", "exec"), ns)
    exec(compile(ast.Module(body=take(REF + "/factory.py", ("load_state_dict",)), type_ignores=[]), REF + "/factory.py", "exec"), ns)
    g = torch.Generator().manual_seed(31)
    out = {}
    width = 48
    for tag, old_grid, new_size, patch in (("up", 7, 160, 16), ("down", 14, 96, 16), ("same", 6, 96, 16)):
        vis = T.VisionTransformer(image_size=new_size, patch_size=patch, width=width, layers=1, heads=2, mlp_ratio=2.0, output_dim=16)
        model = types.SimpleNamespace(visual=vis, positional_embedding=torch.zeros(20, 32))
        pe = torch.randn(1 + old_grid * old_grid, width, generator=g)
        sd = {"visual.positional_embedding": pe.clone(), "positional_embedding": torch.randn(77, 32, generator=g)}
        out[f"vis_{tag}/in"] = pe
        out[f"txt_{tag}/in"] = sd["positional_embedding"].clone()
        ns["resize_pos_embed"](sd, model)
        ns["resize_text_pos_embed"](sd, model)
        out[f"vis_{tag}/out"] = sd["visual.positional_embedding"]
        out[f"vis_{tag}/new_grid"] = np.array(vis.grid_size)
        out[f"txt_{tag}/out"] = sd["positional_embedding"]
    flat = {"text_projection": 1, "positional_embedding": 2, "token_embedding.weight": 3, "transformer.resblocks.0.ln_1.weight": 4,
            "ln_final.bias": 5, "visual.proj": 6, "logit_scale": 7}
    conv = ns["convert_to_custom_text_state_dict"](dict(flat))
    out["custom_text/in_keys"] = np.array(list(flat))
    out["custom_text/out_keys"] = np.array(list(conv))
    with tempfile.TemporaryDirectory() as d:
        tensors = {"a.weight": torch.arange(6.).reshape(2, 3), "b": torch.tensor(2.5)}
        layouts = {"bare": tensors, "train": {"epoch": 3, "name": "x", "state_dict": tensors, "optimizer": {}},
                   "ddp": {"epoch": 1, "state_dict": {"module." + k: v for k, v in tensors.items()}}}
        for name, blob in layouts.items():
            path = os.path.join(d, name + ".pt")
            torch.save(blob, path)
            got = ns["load_state_dict"](path)
            out[f"load/{name}/keys"] = np.array(list(got))
            for k, v in got.items():
                out[f"load/{name}/value/{k}"] = v
    save("checkpoint_interop.npz", **out)


def golden_retrieval():
    """the reference's `compute_retrieval` and `remap_indices` (train.py:429-508).  train.py cannot be imported
    (open_clip_train), so the two functions are taken out of its source with `ast` and executed as they stand (they need
    only torch and numpy).  Stored: a similarity matrix with COCO-like structure (5 captions per image, shuffled dataset image
    ids), the id dictionaries as arrays, the remapped dictionaries and all ten metrics."""
    import ast
    src = open(REF + "/train.py").read()
    fns = [n for n in ast.parse(src).body if isinstance(n, ast.FunctionDef) and n.name in ("compute_retrieval", "remap_indices")]
    ns = {"torch": torch, "np": np}
    exec(compile(ast.Module(body=fns, type_ignores=[]), REF + "/train.py", "exec"), ns)
    g = torch.Generator().manual_seed(21)
    out = {}
    for tag, n_img, k, e in (("a", 40, 5, 32), ("b", 128, 5, 64)):
        n_txt = n_img * k
        fi = F.normalize(torch.randn(n_img, e, generator=g), dim=-1)
        ft = F.normalize(fi.repeat_interleave(k, 0) * 0.35 + torch.randn(n_txt, e, generator=g), dim=-1)   # weakly aligned
        sim = 14.0 * fi @ ft.t()
        img_ids = 500 + 3 * torch.randperm(n_img, generator=g)
        cap_ids = torch.arange(n_txt)
        owner = torch.arange(n_txt) // k
        img2txt = {int(img_ids[i]): [int(c) for c in cap_ids[owner == i]] for i in range(n_img)}
        txt2img = {int(c): [int(img_ids[owner[c]])] for c in range(n_txt)}
        new_i2t, new_t2i = ns["remap_indices"](merged_img_ids=img_ids, cap_ids=cap_ids, img2txt_dict=img2txt, txt2img_dict=txt2img)
        metrics = ns["compute_retrieval"](sim, new_t2i, new_i2t)
        out.update({f"{tag}/image_features": fi, f"{tag}/text_features": ft, f"{tag}/similarity": sim, f"{tag}/img_ids": img_ids,
                    f"{tag}/cap_ids": cap_ids, f"{tag}/captions_per_image": np.array(k),
                    f"{tag}/remapped_txt2img": np.array([new_t2i[c] for c in range(n_txt)]),
                    f"{tag}/remapped_img2txt": np.array([new_i2t[i] for i in range(n_img)]),
                    f"{tag}/metric_names": np.array(list(metrics.keys())),
                    f"{tag}/metric_values": np.array([float(v) for v in metrics.values()])})
    save("retrieval.npz", **out)


def build_ref_colxlip(T, cfg, sd, alpha):
    """The reference's ColXLIP methods on the reference's towers (SURVEY 8f-2, round-3 review item 1).

    `model.py` imports open_clip at module level and `ColXLIP` subclasses open_clip's `CLIP`, so the class cannot be
    imported or instantiated.  Its three METHODS -- `encode_image`, `encode_text`, `forward` (model.py:532-609,631-687) --
    touch only attributes that the importable `transformer.py` can supply, so they are taken out of the class body with
    `ast`, executed unchanged, and bound to a holder module whose attributes are the reference's own objects:
    `visual` = VisionTransformer(output_tokens=True) (what ColXLIP.__init__ sets at model.py:493,510); `transformer`,
    `token_embedding`, `positional_embedding`, `attn_mask`, `ln_final`, `text_projection` = the members of the reference's
    TextTransformer (open_clip's CLIP.__init__ moves exactly these out of its text tower); `text_pool_type` = its
    `pool_type`; the two heads = nn.Sequential(LayerNorm, Linear, GELU, LayerNorm) as model.py:518-530 builds them."""
    import ast
    nn = torch.nn
    tree = ast.parse(open(REF + "/model.py").read())
    klass = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "ColXLIP")
    fns = [n for n in klass.body if isinstance(n, ast.FunctionDef) and n.name in ("encode_image", "encode_text", "forward")]
    assert len(fns) == 3
    from typing import Optional
    ns = {"torch": torch, "nn": nn, "F": F, "Optional": Optional, "text_global_pool": T.text_global_pool}
    exec(compile(ast.Module(body=fns, type_ignores=[]), REF + "/model.py", "exec"), ns)

    vis, txt = build_ref_towers(T, cfg, {k: v for k, v in sd.items() if "token_layer" not in k})
    vis.output_tokens = True

    class Holder(nn.Module):
        encode_image = ns["encode_image"]
        encode_text = ns["encode_text"]
        forward = ns["forward"]

    m = Holder()
    m.visual = vis
    m.transformer = txt.transformer
    m.token_embedding = txt.token_embedding
    m.positional_embedding = txt.positional_embedding
    m.register_buffer("attn_mask", txt.attn_mask, persistent=False)
    m.ln_final = txt.ln_final
    m.text_projection = txt.text_projection
    m.text_pool_type = txt.pool_type
    m.logit_scale = nn.Parameter(sd["logit_scale"].clone())
    m.logit_bias = None
    m.alpha = alpha
    m.vision_token_layer = nn.Sequential(nn.LayerNorm(cfg.vision_width), nn.Linear(cfg.vision_width, cfg.embed_dim),
                                         nn.GELU(), nn.LayerNorm(cfg.embed_dim))
    m.text_token_layer = nn.Sequential(nn.LayerNorm(cfg.text_width), nn.Linear(cfg.text_width, cfg.embed_dim),
                                       nn.GELU(), nn.LayerNorm(cfg.embed_dim))
    missing = m.load_state_dict({k: v for k, v in sd.items()}, strict=True)
    assert not missing.missing_keys and not missing.unexpected_keys
    assert sorted(k for k, _ in m.named_parameters()) == sorted(sd.keys())      # the state-dict schema IS the reference's
    m.train()
    return m


COLXLIP = {
    # tag: (config dir, model name, batch, alpha)
    "colxlip_small": (os.path.join(ROOT, "tests", "model_configs"), "ViT-small-test-colxlip", 8, 0.4),
    # the only ColXLIP architecture the reference ships (model_configs/ViT-B-16-colxlip.json), full width and depth
    # (batch 8: as for the round-3 CLIP fixtures, no gradient is a remainder of two cancelling samples)
    "colxlip_b16": (os.path.join(ROOT, "colxlip_amd", "model_configs"), "ViT-B-16-colxlip", 8, 0.5),
}


def golden_colxlip(T, L, tag):
    """ColXLIP.forward (reference methods, executed) -> the reference's ColClipLoss -> backward.  Both fixtures store
    the four feature tensors, the three losses, the token logits and every gradient as norm + 128 strided elements +
    CountSketch; weights and inputs are regenerated from their seeds by the consumer (checksummed).  `colxlip_small` also
    keeps the image and, in full, every gradient of at most 16 Ki elements (all head, LayerNorm, bias and attention
    parameters)."""
    import json
    cfg_dir, model_name, batch, alpha = COLXLIP[tag]
    with open(os.path.join(cfg_dir, model_name + ".json")) as f:
        cfg = O.ClipCfg.from_model_json(json.load(f))
    sd = O.colxlip_state_dict(cfg)
    image, text = O.synthetic_batch(cfg, batch, seed=4321)
    m = build_ref_colxlip(T, cfg, sd, alpha)
    out = m(image, text)
    assert set(out) == {"image_features", "text_features", "token_image_features", "token_text_features", "logit_scale"}
    res = L.ColClipLoss(alpha=alpha)(**out, output_dict=True)
    res["total_loss"].backward()
    grads = {k: (p.grad if p.grad is not None else torch.zeros_like(p)) for k, p in m.named_parameters()}
    # encode_* with normalize=False (what retrieval evaluation calls, train.py:533,600): the un-normalised pair
    with torch.no_grad():
        pi, ti_raw = m.encode_image(image, normalize=False)
        pt, tt_raw = m.encode_text(text, normalize=False)
    arrs = {"alpha": np.array(alpha), "batch": np.array(batch), "data_seed": np.array(4321),
            "image_features": out["image_features"], "text_features": out["text_features"],
            "token_image_features": out["token_image_features"], "token_text_features": out["token_text_features"],
            "logit_scale": out["logit_scale"], "image_pooled": pi, "text_pooled": pt,
            "token_image_raw_head0": ti_raw[0], "token_text_raw_head0": tt_raw[0],
            "global_loss": res["global_contrastive_loss"], "token_loss": res["token_contrastive_loss"],
            "total_loss": res["total_loss"],
            "logits_per_text_token": L.ColClipLoss().get_logits(out["image_features"], out["text_features"],
                                                                out["token_image_features"], out["token_text_features"],
                                                                out["logit_scale"])["logits_per_text_token"]}
    names = sorted(grads.keys())
    arrs["grad_names"] = np.array(names)
    arrs["grad_norms"] = np.array([float(grads[k].double().norm()) for k in names])
    arrs["sd_checksum"] = np.array([float(sd[k].double().sum()) for k in sorted(sd.keys())])
    arrs["text"] = text
    arrs["grad_sample"] = np.stack([
        F.pad(grads[k].reshape(-1)[grad_sample_index(grads[k].numel())], (0, max(0, GRAD_SAMPLE - grads[k].numel()))).numpy()
        for k in names])
    arrs["grad_sketch"] = np.stack([O.count_sketch(grads[k]).numpy() for k in names])
    if tag != "colxlip_small":         # 8 x 196 x 512 image-token features: every 4th token of every image is kept
        arrs["token_image_features_s4"] = arrs.pop("token_image_features")[:, ::4]
    if tag == "colxlip_small":         # small enough to also keep the image and every gradient of <= 16 Ki elements in full
        arrs["image"] = image
        for k, v in grads.items():
            if v.numel() <= 16384:
                arrs["grad/" + k] = v
    save(f"{tag}_batch{batch}.npz", **arrs)


SEAM_SIGNATURES = [
    ("colxlip/factory.py", None, "create_model"),
    ("colxlip/factory.py", None, "create_model_and_transforms"),
    ("colxlip/factory.py", None, "create_loss"),
    ("colxlip/factory.py", None, "get_tokenizer"),
    ("colxlip/factory.py", None, "load_checkpoint"),
    ("colxlip/factory.py", None, "load_state_dict"),
    ("colxlip/loss.py", None, "gather_features"),
    ("colxlip/loss.py", None, "compute_colbert_similarity"),
    ("colxlip/loss.py", "ClipLoss", "__init__"),
    ("colxlip/loss.py", "ClipLoss", "get_ground_truth"),
    ("colxlip/loss.py", "ClipLoss", "get_logits"),
    ("colxlip/loss.py", "ClipLoss", "forward"),
    ("colxlip/loss.py", "ColClipLoss", "__init__"),
    ("colxlip/train.py", None, "train_one_epoch"),
    ("colxlip/train.py", None, "evaluate"),
    ("colxlip/train.py", None, "compute_retrieval"),
    ("colxlip/train.py", None, "retrieval_on_split"),
    ("colxlip/data.py", None, "get_data"),
    ("colxlip/params.py", None, "parse_args"),
    ("colxlip/model.py", None, "convert_weights_to_lp"),
    ("colxlip/model.py", None, "get_cast_dtype"),
    ("colxlip/model.py", None, "get_input_dtype"),
]


def golden_seam():
    """what the reference's entry point imports from `colxlip`, which `args.<flag>` its main() and train loop read
    and set, and the parameter lists of the functions it calls -- read from the reference's files with `ast` (nothing is
    executed) and stored as names only, so that tests/test_seam_cpu.py checks the seam without the reference present."""
    import ast
    import json
    src = os.path.dirname(REF)

    def tree(rel):
        with open(os.path.join(src, rel)) as f:
            return ast.parse(f.read())

    def func(t, name, cls=None):
        body = t.body
        if cls is not None:
            body = next(n for n in body if isinstance(n, ast.ClassDef) and n.name == cls).body
        return next(n for n in body if isinstance(n, ast.FunctionDef) and n.name == name)

    def args_attrs(node, ctx):
        return sorted({n.attr for n in ast.walk(node) if isinstance(n, ast.Attribute) and isinstance(n.value, ast.Name)
                       and n.value.id == "args" and isinstance(n.ctx, ctx)})

    def literal_defaults(fn):
        out = {}
        for name, node in zip(reversed([x.arg for x in fn.args.args]), reversed(fn.args.defaults)):
            try:
                ast.literal_eval(node)
            except ValueError:
                continue          # torch.float16 etc.
            out[name] = ast.unparse(node)
        return out

    main_tree = tree("main.py")
    main_fn = func(main_tree, "main")
    train_tree = tree("colxlip/train.py")
    seam = {
        "main_colxlip_imports": [{"module": n.module, "names": [a.name for a in n.names], "line": n.lineno}
                                 for n in ast.walk(main_tree)
                                 if isinstance(n, ast.ImportFrom) and n.module and n.module.split(".")[0] == "colxlip"],
        "root_exports": [a.name for n in ast.walk(tree("colxlip/__init__.py")) if isinstance(n, ast.ImportFrom) for a in n.names],
        "main_args_read": args_attrs(main_fn, ast.Load),
        "main_args_set": args_attrs(main_fn, ast.Store),
        "train_args_read": {fn: args_attrs(func(train_tree, fn), ast.Load)
                            for fn in ("train_one_epoch", "evaluate", "retrieval_on_split")},
        "signatures": {},
    }
    for rel, cls, fn in SEAM_SIGNATURES:
        node = func(tree(rel), fn, cls)
        a = node.args
        seam["signatures"][f"{rel}:{cls + '.' if cls else ''}{fn}"] = {
            "params": [x.arg for x in a.posonlyargs + a.args + a.kwonlyargs],
            "var_keyword": a.kwarg is not None,
            "literal_defaults": literal_defaults(node),
        }
    path = os.path.join(HERE, "seam.json")
    with open(path, "w") as f:
        json.dump(seam, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"wrote seam.json: {os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    if sys.argv[1:] == ["seam"]:       # text only: nothing of the reference is imported
        golden_seam()
        sys.exit(0)
    torch.manual_seed(0)
    torch.set_num_threads(8)
    T, L = import_reference()
    if len(sys.argv) > 1:              # e.g. `make_golden.py b16 l14_336 h14 lp`: only the named fixtures
        for tag in sys.argv[1:]:
            if tag in COLXLIP:
                golden_colxlip(T, L, tag)
            elif tag == "lp":
                golden_lp(T)
            elif tag == "retrieval":
                golden_retrieval()
            elif tag == "checkpoint":
                golden_checkpoint(T)
            elif tag == "colclip_dist":
                golden_colclip_dist()
            else:
                golden_real_size(T, L, tag)
        sys.exit(0)
    golden_tiny_clip(T, L)
    golden_loss_w1(L)
    golden_colclip_loss(L)
    golden_misc(T, L)
    golden_loss_dist()
    golden_colclip_dist()
    golden_lp(T)
    golden_retrieval()
    golden_checkpoint(T)
    for tag in COLXLIP:
        golden_colxlip(T, L, tag)
    for tag in REAL_SIZE:
        golden_real_size(T, L, tag)
