"""Generate the ViT-B-32-colxlip fixture: the architecture the reference's ColXLIP launch line names (src/colxlip.sh:38,
`--model ViT-B-32-colxlip --alpha 0.7`; 49 image tokens), stepped once by the reference's own `ColXLIP.encode_image /
encode_text / forward` and `ColClipLoss` at batch 8.

Like make_golden.py (whose helpers it imports), this runs only where the reference tree is available; the fixture is data only.
Format of colxlip_b16_batch8.npz, with BOTH token feature tensors strided (every 4th token) and without the un-normalised
head rows, which keeps the file below 1 MiB.

    python tests/golden/make_golden_colxlip_b32.py
"""
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from make_golden import GRAD_SAMPLE, ROOT, O, build_ref_colxlip, grad_sample_index, import_reference, save  # noqa: E402

MODEL, BATCH, ALPHA, DATA_SEED = "ViT-B-32-colxlip", 8, 0.7, 4321


def main():
    T, L = import_reference()
    torch.manual_seed(0)
    with open(os.path.join(ROOT, "colxlip_amd", "model_configs", MODEL + ".json")) as f:
        cfg = O.ClipCfg.from_model_json(json.load(f))
    sd = O.colxlip_state_dict(cfg)
    image, text = O.synthetic_batch(cfg, BATCH, seed=DATA_SEED)
    m = build_ref_colxlip(T, cfg, sd, ALPHA)
    out = m(image, text)
    assert out["token_image_features"].shape == (BATCH, 49, cfg.embed_dim)
    res = L.ColClipLoss(alpha=ALPHA)(**out, output_dict=True)
    res["total_loss"].backward()
    grads = {k: (p.grad if p.grad is not None else torch.zeros_like(p)) for k, p in m.named_parameters()}
    names = sorted(grads.keys())
    arrs = {"alpha": np.array(ALPHA), "batch": np.array(BATCH), "data_seed": np.array(DATA_SEED),
            "image_features": out["image_features"], "text_features": out["text_features"],
            "token_image_features_s4": out["token_image_features"][:, ::4], "token_text_features_s4": out["token_text_features"][:, ::4],
            "logit_scale": out["logit_scale"],
            "global_loss": res["global_contrastive_loss"], "token_loss": res["token_contrastive_loss"], "total_loss": res["total_loss"],
            "logits_per_text_token": L.ColClipLoss().get_logits(out["image_features"], out["text_features"],
                                                                out["token_image_features"], out["token_text_features"],
                                                                out["logit_scale"])["logits_per_text_token"],
            "grad_names": np.array(names),
            "grad_norms": np.array([float(grads[k].double().norm()) for k in names]),
            "sd_checksum": np.array([float(sd[k].double().sum()) for k in sorted(sd.keys())]),
            "text": text,
            "grad_sample": np.stack([
                F.pad(grads[k].reshape(-1)[grad_sample_index(grads[k].numel())], (0, max(0, GRAD_SAMPLE - grads[k].numel()))).numpy()
                for k in names]),
            "grad_sketch": np.stack([O.count_sketch(grads[k]).numpy() for k in names])}
    save("colxlip_b32_batch8.npz", **arrs)


if __name__ == "__main__":
    main()
