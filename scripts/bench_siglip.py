"""Time SigLipLoss forward + backward (csrc/loss_sigmoid.hip) at E = 512 and print TFLOP/s against its 4 logits-GEMM equivalents
(2 * N * N * E FLOP each), with ClipLoss's fused path (5 equivalents) at the same shapes as the yardstick.  One GPU, W = 1.
    python scripts/bench_siglip.py [N ...]"""
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from colxlip_amd.loss import ClipLoss, SigLipLoss  # noqa: E402


def timed(step, iters):
    for _ in range(3):
        step()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        step()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


e = 512
dev = "cuda"
for N in [int(a) for a in sys.argv[1:]] or [1024, 4096, 16384]:
    g = torch.Generator(device=dev).manual_seed(0)
    fi = torch.nn.functional.normalize(torch.randn(N, e, device=dev, generator=g), dim=-1).requires_grad_(True)
    ft = torch.nn.functional.normalize(torch.randn(N, e, device=dev, generator=g), dim=-1).requires_grad_(True)
    ls = torch.tensor(math.log(10.0), device=dev, requires_grad=True)
    lb = torch.tensor(-10.0, device=dev, requires_grad=True)
    sig, clip = SigLipLoss(), ClipLoss()

    def sig_step():
        for t in (fi, ft, ls, lb):
            t.grad = None
        sig(fi, ft, ls.exp(), lb).backward()

    def clip_step():
        for t in (fi, ft, ls):
            t.grad = None
        clip(fi, ft, ls.exp()).backward()

    def sig_nograd():
        with torch.no_grad():
            sig(fi, ft, ls.exp(), lb)

    iters = 20 if N <= 4096 else 5
    ms_sig, ms_clip, ms_ng = timed(sig_step, iters), timed(clip_step, iters), timed(sig_nograd, iters)
    gemm = 2.0 * N * N * e
    print(f"N={N} E={e}: SigLipLoss fwd+bwd {ms_sig:.3f} ms ({4 * gemm / ms_sig / 1e9:.1f} TFLOP/s on 4 GEMM-equivalents) | "
          f"no_grad fwd {ms_ng:.3f} ms ({gemm / ms_ng / 1e9:.1f} TFLOP/s) | ClipLoss fused fwd+bwd {ms_clip:.3f} ms "
          f"({5 * gemm / ms_clip / 1e9:.1f} TFLOP/s on 5)", flush=True)
