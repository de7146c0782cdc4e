"""Time DistillClipLoss (csrc/loss_distill.hip) and distillation in the train step, bf16, one GPU, W = 1.

  loss   forward + backward of the fused loss at N = 4096 for (Es, Et) = (512, 512) and (512, 768), against ClipLoss's fused
         path on the same features (FLOP: 2 * N * N * E per logits-GEMM equivalent; ClipLoss runs 5 at Es, DistillClipLoss
         one at Es + Et in the forward and 2 x (Es + Et + Es) in the backward)
  step   the full train step (forward, loss, backward, FusedAdamW) of a ViT-B/32 student at b = 4096 with a ViT-B/16 teacher
         (random weights through a temporary checkpoint, as `--distill-pretrained` loads them), against the same step without
         a teacher, and the teacher forward alone (its share of the step)

    python scripts/bench_distill.py [--steps 10] [--warmup 3] [--skip-step]"""
import argparse
import json
import math
import os
import sys
import tempfile

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from colxlip_amd import create_model, create_model_and_transforms, ops  # noqa: E402
from colxlip_amd.data import synthetic_batch  # noqa: E402
from colxlip_amd.loss import ClipLoss, DistillClipLoss  # noqa: E402
from colxlip_amd.optim import FusedAdamW, param_groups  # noqa: E402


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


def bench_loss(n, es, et, steps, warmup):
    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(0)
    nz = torch.nn.functional.normalize
    fi = nz(torch.randn(n, es, device=dev, generator=g), dim=-1).requires_grad_(True)
    ft = nz(torch.randn(n, es, device=dev, generator=g), dim=-1).requires_grad_(True)
    tfi = nz(torch.randn(n, et, device=dev, generator=g), dim=-1)
    tft = nz(torch.randn(n, et, device=dev, generator=g), dim=-1)
    ls = torch.tensor(math.log(10.0), device=dev, requires_grad=True)
    tscale = torch.tensor(50.0, device=dev)
    dl, cl = DistillClipLoss(), ClipLoss()

    def distill_step():
        for t in (fi, ft, ls):
            t.grad = None
        c, d = dl(fi, ft, ls.exp(), tfi, tft, tscale)
        (c + d).backward()

    def clip_step():
        for t in (fi, ft, ls):
            t.grad = None
        cl(fi, ft, ls.exp()).backward()

    ms_d, ms_c = timed(distill_step, steps, warmup), timed(clip_step, steps, warmup)
    flop_d = 2.0 * n * n * (5 * es + 3 * et)       # fwd: s + t tiles; bwd: two walks of (s + t tiles + the product at Es)
    flop_c = 2.0 * n * n * es * 5
    return {"bench": "loss", "N": n, "Es": es, "Et": et, "distill_fwd_bwd_ms": round(ms_d, 3),
            "distill_tflops": round(flop_d / ms_d / 1e9, 1), "clip_fused_fwd_bwd_ms": round(ms_c, 3),
            "clip_tflops": round(flop_c / ms_c / 1e9, 1), "ratio_vs_clip": round(ms_d / ms_c, 3)}


def bench_step(b, steps, warmup):
    dev = "cuda"
    torch.manual_seed(0)
    model, _, _ = create_model_and_transforms("ViT-B-32", precision="bf16", device=dev, output_dict=True)
    model.train()
    with tempfile.TemporaryDirectory() as d:
        torch.manual_seed(1)
        ckpt = os.path.join(d, "teacher.pt")
        torch.save(create_model("ViT-B-16", precision="fp32", device="cpu").state_dict(), ckpt)
        teacher = create_model("ViT-B-16", ckpt, precision="bf16", device=dev, output_dict=True)
    teacher.eval()
    images, texts = synthetic_batch(b, model.visual.image_size, model.context_length, model.vocab_size, seed=1234, device=dev,
                                    image_dtype=torch.bfloat16)
    texts = texts[:, 0].contiguous()
    opt = FusedAdamW(param_groups(model.named_parameters(), 0.2), lr=1e-5, betas=(0.9, 0.98), eps=1e-6)
    clip, distill = ClipLoss(cache_labels=True), DistillClipLoss(cache_labels=True)

    def step(with_teacher):
        opt.zero_grad(set_to_none=True)
        if with_teacher:
            with torch.no_grad():
                tout = teacher(images, texts)
        out = model(images, texts)
        if with_teacher:
            out.update({f"dist_{k}": v for k, v in tout.items()})
            losses = distill(**out, output_dict=True)
            total = losses["contrastive_loss"] + losses["distill_loss"]
        else:
            total = clip(**out)
        total.backward()
        opt.step()
        ops.clamp1(model.logit_scale.data, 0.0, math.log(100))

    def teacher_fwd():
        with torch.no_grad():
            teacher(images, texts)

    plain = timed(lambda: step(False), steps, warmup)
    with_t = timed(lambda: step(True), steps, warmup)
    tfwd = timed(teacher_fwd, steps, warmup)
    return {"bench": "step", "student": "ViT-B-32", "teacher": "ViT-B-16", "batch": b, "precision": "bf16",
            "step_ms_no_teacher": round(plain, 2), "step_ms_with_teacher": round(with_t, 2),
            "teacher_fwd_ms": round(tfwd, 2), "teacher_fwd_share_of_step": round(tfwd / with_t, 3),
            "images_per_s_no_teacher": round(b / plain * 1e3, 1), "images_per_s_with_teacher": round(b / with_t * 1e3, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--skip-step", action="store_true")
    a = ap.parse_args()
    for es, et in ((512, 512), (512, 768)):
        print(json.dumps(bench_loss(4096, es, et, 2 * a.steps, a.warmup)), flush=True)
    if not a.skip_step:
        print(json.dumps(bench_step(4096, a.steps, a.warmup)), flush=True)


if __name__ == "__main__":
    main()
