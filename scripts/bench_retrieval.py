"""Late-interaction retrieval scoring at ViT-B-16-colxlip token shapes (q = 196 image tokens, n = 77 text tokens, E = 512, bf16;
text shaped like ColXLIP's output: every position at / behind an EOT ~ U[8, 76] is one vector).

  a  N x N (default 512, the training shape): `ops.maxsim_scores` against `_MaxSimFused.forward` (gemm + finish + mean, the
     only route before the forward-only scorer) on the same tensors, alternating, REPEATS times each: time and peak allocated
     memory above the inputs, and the largest difference of the two results.
  b  a COCO-shaped gallery (default 5000 images x 25000 captions): scoring time, achieved TFLOP/s of the MaxSim GEMM counted on
     the packed rows (2 * R * ni * q * E), peak memory; next to it the in-training figure of the same GEMM (the N x N forward).
  c  `evaluate()` of ViT-B-16-colxlip (bf16) on the synthetic split of the same size, split into encode and score.

    python scripts/bench_retrieval.py [a] [b] [c] [--n 512] [--images 5000] [--captions-per-image 5] [--repeats 5]
One JSON line per part on stdout."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from colxlip_amd import ops  # noqa: E402
from colxlip_amd.loss import _MaxSimFused  # noqa: E402

Q, N_TOK, E = 196, 77, 512
DEV = "cuda"


def tokens(ni, nt, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    ti = torch.empty((ni, Q, E), dtype=torch.bfloat16, device=DEV)
    for k0 in range(0, ni, 512):
        ti[k0:k0 + 512] = torch.nn.functional.normalize(torch.randn(min(512, ni - k0), Q, E, device=DEV, generator=g), dim=-1).bfloat16()
    tt = torch.empty((nt, N_TOK, E), dtype=torch.bfloat16, device=DEV)
    tail = torch.nn.functional.normalize(torch.randn(E, device=DEV, generator=g), dim=-1).bfloat16()
    for m0 in range(0, nt, 1024):
        c = min(1024, nt - m0)
        blk = torch.nn.functional.normalize(torch.randn(c, N_TOK, E, device=DEV, generator=g), dim=-1).bfloat16()
        eot = torch.randint(8, N_TOK, (c,), device=DEV, generator=g)
        blk[torch.arange(N_TOK, device=DEV).unsqueeze(0) >= eot.unsqueeze(1)] = tail
        tt[m0:m0 + c] = blk
    return ti, tt


def timed(fn):
    """(milliseconds, peak bytes allocated above what was live before the call, result)"""
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), torch.cuda.max_memory_allocated() - base, out


def spread(xs):
    xs = sorted(xs)
    return {"min": round(xs[0], 3), "median": round(xs[len(xs) // 2], 3), "max": round(xs[-1], 3)}


def part_a(n, repeats):
    ti, tt = tokens(n, n, 0)
    G = torch.randn(n, n, device=DEV)

    def new():
        return ops.maxsim_scores(ti, tt, G, 0.5, 14.0)

    def old():
        with torch.no_grad():
            return _MaxSimFused.forward(_Ctx(), ti, tt)

    for _ in range(2):
        new(), old()
    t_new, t_old, m_new, m_old = [], [], 0, 0
    for _ in range(repeats):
        ms, mem, s = timed(new)
        t_new.append(ms)
        m_new = max(m_new, mem)
        ms, mem, lg = timed(old)
        t_old.append(ms)
        m_old = max(m_old, mem)
    diff = float((s - 14.0 * (0.5 * G + 0.5 * lg.t())).abs().max())
    cu, R = ops.maxsim_pack_text(tt)
    ld = (R + 255) // 256 * 256
    return {"part": "a", "n": n, "packed_rows": R, "repeats": repeats, "maxsim_scores_ms": spread(t_new), "maxsim_fused_forward_ms": spread(t_old),
            "maxsim_scores_peak_MiB": round(m_new / 2**20, 1), "maxsim_fused_forward_peak_MiB": round(m_old / 2**20, 1),
            "maxvT_argT_inv_count_MiB": round((n * ld * 6 + n * n * 4) / 2**20, 1), "max_abs_difference_of_scores": diff,
            "gemm_tflops_in_training_forward": round(2.0 * R * n * Q * E / (sorted(t_old)[len(t_old) // 2] * 1e-3) / 1e12, 1)}


class _Ctx:
    def save_for_backward(self, *tensors):
        pass


def part_b(ni, per, repeats):
    nt = ni * per
    ti, tt = tokens(ni, nt, 1)
    G = torch.randn(ni, nt, device=DEV)
    out = torch.empty((ni, nt), dtype=torch.float32, device=DEV)
    ops.maxsim_scores(ti, tt, G, 0.5, 14.0, out=out)
    ts, peak = [], 0
    for _ in range(repeats):
        ms, mem, _ = timed(lambda: ops.maxsim_scores(ti, tt, G, 0.5, 14.0, out=out))
        ts.append(ms)
        peak = max(peak, mem)
    _, R = ops.maxsim_pack_text(tt)
    med = sorted(ts)[len(ts) // 2]
    flop = 2.0 * R * ni * Q * E
    return {"part": "b", "images": ni, "captions": nt, "packed_rows": R, "repeats": repeats, "scoring_ms": spread(ts),
            "gemm_flop": flop, "tflops_whole_scoring_call": round(flop / (med * 1e-3) / 1e12, 1),
            "peak_MiB_above_inputs_and_scores": round(peak / 2**20, 1),
            "maxvT_argT_the_training_route_would_hold_GiB": round(ni * R * 6 / 2**30, 1)}


def part_c(ni, per):
    from colxlip_amd import create_model_and_transforms
    from colxlip_amd import train as TR
    from colxlip_amd.data import synthetic_retrieval_split
    from colxlip_amd.params import parse_args
    model, _, _ = create_model_and_transforms("ViT-B-16-colxlip", precision="bf16", device=DEV, output_dict=True)
    args = parse_args(["--model", "ViT-B-16-colxlip", "--dataset-type", "synthetic", "--precision", "bf16", "--alpha", "0.5"])
    args.rank, args.local_rank, args.world_size, args.distributed, args.device = 0, 0, 1, False, DEV
    args.save_logs, args.wandb = False, False
    split = synthetic_retrieval_split(ni, per, 224, 77, getattr(model, "vocab_size", 49408), seed=3, device=DEV, batch_size=500, image_dtype=torch.bfloat16)
    txt, img, _, _ = split
    small = synthetic_retrieval_split(64, per, 224, 77, getattr(model, "vocab_size", 49408), seed=4, device=DEV, batch_size=64, image_dtype=torch.bfloat16)
    TR.evaluate(model, {"retrieval_coco": small}, 1, args)                      # warm-up of every kernel family
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    model.eval()
    found = TR.encode_split(model, txt.dataloader, img.dataloader, torch.device(DEV), torch.bfloat16, with_tokens=True)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    with torch.no_grad():
        G = TR.similarity_matrix(found[0], found[2])
        ops.maxsim_scores(found[4], found[5], G, 0.5, float(model.logit_scale.exp()))
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    del found, G
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    metrics = TR.evaluate(model, {"retrieval_coco": split}, 1, args)
    torch.cuda.synchronize()
    t3 = time.perf_counter()
    return {"part": "c", "images": ni, "captions": ni * per, "encode_s": round(t1 - t0, 2), "score_s": round(t2 - t1, 2),
            "evaluate_wall_s": round(t3 - t2, 2), "evaluate_peak_GiB": round(torch.cuda.max_memory_allocated() / 2**30, 1),
            "text_to_image_R@1": metrics["retrieval_coco_text_to_image_R@1"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("parts", nargs="*", default=["a", "b", "c"])
    ap.add_argument("--n", type=int, default=512)
    ap.add_argument("--images", type=int, default=5000)
    ap.add_argument("--captions-per-image", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_retrieval.py measures on the GPU; there is none here")
    for part in a.parts:
        res = {"a": lambda: part_a(a.n, a.repeats), "b": lambda: part_b(a.images, a.captions_per_image, a.repeats),
               "c": lambda: part_c(a.images, a.captions_per_image)}[part]()
        print(json.dumps(res), flush=True)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
