"""Time the token-level (MaxSim) part of ColClipLoss and the forward-only scorer at ViT-B/32-colxlip shapes -- n = 77 text tokens,
q = 49 image tokens (--q), E = 512 -- on the fused route (csrc/gemm_nt_maxsim.h for q < 64) against the unfused one
(CLIPX_MAXSIM_FUSED=0: the similarity matrix written, reduced by a second kernel; fp32 gemm_f32 for the scorer).

Per N three measurements, each with both routes ALTERNATING inside this process, every shape warmed up first, >= 20 timed
iterations per arm, median and min .. max of each arm:
  * ColClipLoss forward + backward on text without duplicates;
  * the same on text shaped like ColXLIP's output (every position at / behind an EOT ~ U[8, 76] is one vector);
  * `ops.maxsim_scores` (forward only, N images x N texts, EOT-shaped text).
Uses only ColClipLoss, compute_colbert_similarity and ops.maxsim_scores.

    python scripts/bench_maxsim_small.py [--q 49] [--iters 20] [N ...]"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from colxlip_amd import ops  # noqa: E402
from colxlip_amd.loss import ColClipLoss, compute_colbert_similarity  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--q", type=int, default=49)
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("N", type=int, nargs="*")
args = ap.parse_args()
assert torch.cuda.is_available(), "bench_maxsim_small.py measures on the GPU"
dev = "cuda"
n, q, e = 77, args.q, 512


def one(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def ab(fn, iters):
    """{arm: [ms]}: arms "0" (unfused) and "1" (fused) alternate, iteration by iteration, after two warm-up calls each"""
    times = {"0": [], "1": []}
    for arm in ("0", "1"):
        os.environ["CLIPX_MAXSIM_FUSED"] = arm
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    for _ in range(iters):
        for arm in ("0", "1"):
            os.environ["CLIPX_MAXSIM_FUSED"] = arm
            times[arm].append(one(fn))
    os.environ["CLIPX_MAXSIM_FUSED"] = "1"
    return times


def report(label, times):
    u, f = times["0"], times["1"]
    mu, mf = statistics.median(u), statistics.median(f)
    spread = (max(u) - min(u)) / mu
    print(f"  {label}: unfused median {mu:.3f} ms (min {min(u):.3f} max {max(u):.3f}, spread {100 * spread:.1f} %) | fused median {mf:.3f} ms "
          f"(min {min(f):.3f} max {max(f):.3f}) | unfused / fused = {mu / mf:.2f}x | fused beats the baseline by more than its spread: "
          f"{'yes' if mf < mu * (1 - spread) else 'NO'}", flush=True)


for N in args.N or [128, 256, 512]:
    g = torch.Generator(device=dev).manual_seed(0)
    fi = torch.nn.functional.normalize(torch.randn(N, e, device=dev, generator=g), dim=-1).requires_grad_(True)
    ft = torch.nn.functional.normalize(torch.randn(N, e, device=dev, generator=g), dim=-1).requires_grad_(True)
    ti = torch.nn.functional.normalize(torch.randn(N, q, e, device=dev, generator=g), dim=-1).bfloat16().requires_grad_(True)
    tt = torch.nn.functional.normalize(torch.randn(N, n, e, device=dev, generator=g), dim=-1).bfloat16().requires_grad_(True)
    ls = torch.tensor(14.0, device=dev, requires_grad=True)
    loss = ColClipLoss(alpha=0.7)
    tail = torch.nn.functional.normalize(torch.randn(e, device=dev, generator=g), dim=-1).bfloat16()
    eot = torch.randint(8, n, (N,), device=dev, generator=g)
    tt_eot = tt.detach().clone()
    tt_eot[torch.arange(n, device=dev).unsqueeze(0) >= eot.unsqueeze(1)] = tail
    tt_eot.requires_grad_(True)

    def step(text_tokens):
        for t in (fi, ft, ti, text_tokens, ls):
            t.grad = None
        loss(image_features=fi, text_features=ft, token_image_features=ti, token_text_features=text_tokens, logit_scale=ls).backward()

    # the two routes compute the same thing: the token logits of both, once, before anything is timed
    with torch.no_grad():
        os.environ["CLIPX_MAXSIM_FUSED"] = "0"
        l0 = compute_colbert_similarity(ti, tt_eot)
        os.environ["CLIPX_MAXSIM_FUSED"] = "1"
        l1 = compute_colbert_similarity(ti, tt_eot)
    print(f"N={N} q={q} n={n} E={e}: S would be {N * n * N * q * 2 / 2**30:.2f} GiB in bf16; max |fused - unfused| token logit "
          f"{float((l0 - l1).abs().max()):.2e}", flush=True)
    report("ColClipLoss fwd+bwd, distinct text rows ", ab(lambda: step(tt), args.iters))
    report(f"ColClipLoss fwd+bwd, EOT-shaped text ({float((eot + 1).float().mean()):.0f} of {n} rows live)", ab(lambda: step(tt_eot), args.iters))
    G = (fi.detach() @ ft.detach().t()).contiguous()
    out = torch.empty((N, N), dtype=torch.float32, device=dev)
    a, b = ti.detach(), tt_eot.detach()
    report("ops.maxsim_scores, EOT-shaped text      ", ab(lambda: ops.maxsim_scores(a, b, G, 0.7, 14.0, out=out), args.iters))
    del fi, ft, ti, tt, tt_eot, G, out, a, b
    torch.cuda.empty_cache()
