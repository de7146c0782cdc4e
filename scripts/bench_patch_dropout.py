"""Time patch dropout (FLIP; `--force-patch-dropout`) in bf16 on one GPU: for ViT-B/32 at b = 4096 and ViT-B/16 at b = 512, at
p = 0, 0.5 and 0.75, the full train step (forward, ClipLoss, backward, FusedAdamW) in ms/step and images/s, and the image tower's
forward + backward alone.  Device events around `--steps` steps after `--warmup`.

    python scripts/bench_patch_dropout.py [--configs b32,b16] [--probs 0,0.5,0.75] [--steps 10] [--warmup 3] [--tower-only]

`--tower-only` times (and runs) only the image tower: the run to put under `rocprofv3 --kernel-trace --stats`, so that every
kernel in the stats belongs to the image tower."""
import argparse
import json
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from colxlip_amd import create_model_and_transforms, ops  # noqa: E402
from colxlip_amd.data import synthetic_batch  # noqa: E402
from colxlip_amd.loss import ClipLoss  # noqa: E402
from colxlip_amd.optim import FusedAdamW, param_groups  # noqa: E402

CONFIGS = {"b32": ("ViT-B-32", 4096), "b16": ("ViT-B-16", 512)}


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="b32,b16")
    ap.add_argument("--probs", default="0,0.5,0.75")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--tower-only", action="store_true")
    a = ap.parse_args()
    dev = "cuda"
    for tag in a.configs.split(","):
        name, b = CONFIGS[tag]
        torch.manual_seed(0)
        model, _, _ = create_model_and_transforms(name, precision="bf16", device=dev, output_dict=True)
        model.train()
        images, texts = synthetic_batch(b, model.visual.image_size, model.context_length, model.vocab_size, seed=1234, device=dev,
                                        image_dtype=torch.bfloat16)
        texts = texts[:, 0].contiguous()
        loss_fn = ClipLoss(cache_labels=True)
        opt = FusedAdamW(param_groups(model.named_parameters(), 0.2), lr=1e-5, betas=(0.9, 0.98), eps=1e-6)
        dfeat = torch.randn(b, model.visual.output_dim, device=dev) * 1e-3
        G2 = model.visual.grid_size[0] * model.visual.grid_size[1]

        def train_step():
            opt.zero_grad(set_to_none=True)
            out = model(images, texts)
            loss_fn(**out).backward()
            opt.step()
            ops.clamp1(model.logit_scale.data, 0.0, math.log(100))

        def tower_step():
            for p in model.visual.parameters():
                p.grad = None
            model.visual(images).backward(dfeat)

        res = {}
        for p in [float(x) for x in a.probs.split(",")]:
            model.visual.patch_dropout.prob = p
            keep = model.visual.patch_dropout.num_keep(G2) if p > 0 else G2
            tower = timed(tower_step, a.steps, a.warmup)
            row = {"model": name, "batch": b, "p": p, "tokens": 1 + keep, "tower_fwd_bwd_ms": round(tower, 3)}
            if not a.tower_only:
                step = timed(train_step, a.steps, a.warmup)
                row.update({"step_ms": round(step, 3), "images_per_s": round(b / step * 1e3, 1)})
            res[p] = row
            print(json.dumps(row), flush=True)
        if 0.0 in res:
            for p, row in res.items():
                if p > 0:
                    msg = {"model": name, "p": p, "tower_time_ratio_vs_p0": round(row["tower_fwd_bwd_ms"] / res[0.0]["tower_fwd_bwd_ms"], 3)}
                    if not a.tower_only:
                        msg["images_per_s_ratio_vs_p0"] = round(row["images_per_s"] / res[0.0]["images_per_s"], 3)
                    print(json.dumps(msg), flush=True)
        del model, opt, images, texts
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
