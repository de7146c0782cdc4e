"""Generate the patch-dropout fixtures by running the reference's own towers with `PatchDropout(p)` (transformer.py:48-88) in
the image tower, then its ClipLoss and the backward.

Like make_golden.py (whose helpers it imports), this runs only where the reference tree is available; the fixture is data
only.  Weights and batch are regenerated from their seeds by the consumer (checksummed).  `torch.manual_seed(seed)` is called
immediately before the image tower's forward, so the mask is the first CPU `randn` that forward draws; the consumer replays it
with the same seed and stores nothing but the kept index to compare against.

    python tests/golden/make_golden_patch_dropout.py
"""
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from make_golden import GRAD_SAMPLE, O, build_ref_towers, grad_sample_index, import_reference, real_size_cfg, save  # noqa: E402

# tag: (model, config directory or None for the product's, batch, prob, dropout seed)
CASES = {
    "small_p50": ("ViT-small-test", os.path.join(os.path.dirname(HERE), "model_configs"), 8, 0.5, 101),
    "small_p75": ("ViT-small-test", os.path.join(os.path.dirname(HERE), "model_configs"), 8, 0.75, 102),
    "b16_p50": ("ViT-B-16", None, 8, 0.5, 103),
}


def _cfg(model_name, cfg_dir):
    if cfg_dir is None:
        return real_size_cfg(model_name)
    with open(os.path.join(cfg_dir, model_name + ".json")) as f:
        return O.ClipCfg.from_model_json(json.load(f))


def golden_patch_dropout_case(T, L, tag):
    model_name, cfg_dir, batch, prob, seed = CASES[tag]
    cfg = _cfg(model_name, cfg_dir)
    sd = O.perturb_state_dict(O.init_state_dict(cfg, seed=0), seed=1)
    image, text = O.synthetic_batch(cfg, batch, seed=1234)
    vis, txt = build_ref_towers(T, cfg, sd)
    vis.patch_dropout = T.PatchDropout(prob)
    vis.train()
    logit_scale = torch.nn.Parameter(sd["logit_scale"].clone())
    torch.manual_seed(seed)
    img_pooled = vis(image)
    txt_pooled = txt(text)
    fi = F.normalize(img_pooled, dim=-1)
    ft = F.normalize(txt_pooled, dim=-1)
    loss = L.ClipLoss()(fi, ft, logit_scale.exp())
    loss.backward()
    grads = {"visual." + k: p.grad for k, p in vis.named_parameters()}
    grads.update({k: p.grad for k, p in txt.named_parameters()})
    grads["logit_scale"] = logit_scale.grad
    # the mask the forward drew: transformer.py:76-80 replayed from the same seed
    G2 = cfg.grid * cfg.grid
    keep = max(1, int(G2 * (1 - prob)))
    torch.manual_seed(seed)
    keep_index = torch.randn(batch, G2).topk(keep, dim=-1).indices
    names = sorted(grads.keys())
    return {
        f"{tag}/prob": np.array(prob), f"{tag}/seed": np.array(seed), f"{tag}/batch": np.array(batch),
        f"{tag}/keep_index": keep_index.numpy().astype(np.int64),
        f"{tag}/image_pooled": img_pooled, f"{tag}/image_features": fi, f"{tag}/text_features": ft, f"{tag}/loss": loss,
        f"{tag}/grad_names": np.array(names),
        f"{tag}/grad_norms": np.array([float(grads[k].double().norm()) for k in names]),
        f"{tag}/grad_maxabs": np.array([float(grads[k].abs().max()) for k in names]),
        f"{tag}/grad_sample": np.stack([F.pad(grads[k].reshape(-1)[grad_sample_index(grads[k].numel())],
                                              (0, max(0, GRAD_SAMPLE - grads[k].numel()))).numpy() for k in names]),
        f"{tag}/grad_sketch": np.stack([O.count_sketch(grads[k]).numpy() for k in names]),
        f"{tag}/sd_checksum": np.array([float(sd[k].double().sum()) for k in sorted(sd.keys())]),
        f"{tag}/batch_checksum": np.array([float(image.double().sum()), float(text.double().sum())]),
    }


if __name__ == "__main__":
    torch.manual_seed(0)
    T, L = import_reference()
    arrs = {}
    for tag in CASES:
        arrs.update(golden_patch_dropout_case(T, L, tag))
    save("patch_dropout.npz", **{k: (v.detach() if isinstance(v, torch.Tensor) else v) for k, v in arrs.items()})
