"""Time two-stage late-interaction search (`LateInteractionIndex.search(candidates=C)`: the C best items per query by the global
similarity, then `clipx_maxsim_pairs` on those only; colxlip_amd/search.py, csrc/maxsim_pairs.hip) against the exhaustive search of
the same index.  The data and shapes of scripts/bench_search.py: 5 000 images x 25 000 captions, q = 49, n = 77, E = 512, bf16,
EOT-shaped text, k = 10, both directions.  All arms ALTERNATE inside this process after two warm-up calls each; every arm reports
median and min .. max.  The two stages are also timed apart with events (stage 1: `similarity_matrix` + `topk_merge` with lists of
length C; stage 2: `rerank`).

Per C the script prints the share of the exhaustive top-10 and top-1 that the two-stage search returns.  The features are random
unit vectors: the global and the token similarities of a pair are INDEPENDENT here, so the global stage picks candidates almost at
random with respect to the final score, and this overlap understates what a trained model (whose global and token similarities
agree) gives.  It is printed to show the code path end to end; no trained model's recall is claimed.

  c. 200 000 images x 2 000 text queries, the large case of bench_search.py.

    python scripts/bench_rerank.py [--iters 20] [--skip-large]"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from colxlip_amd import ops  # noqa: E402
from colxlip_amd.search import LateInteractionIndex  # noqa: E402
from colxlip_amd.train import similarity_matrix  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--skip-large", action="store_true")
args = ap.parse_args()
assert torch.cuda.is_available(), "bench_rerank.py measures on the GPU"
dev = "cuda"
CS = (16, 64, 256)
K = 10


def one(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def alternate(arms, iters):
    times = {name: [] for name in arms}
    for fn in arms.values():
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    for _ in range(iters):
        for name, fn in arms.items():
            times[name].append(one(fn))
    return times


def line(name, t):
    return f"{name} median {statistics.median(t):.3f} ms (min {min(t):.3f} max {max(t):.3f})"


def normal_tokens(n, rows, e, gen):
    return torch.nn.functional.normalize(torch.randn(n, rows, e, device=dev, generator=gen), dim=-1).bfloat16()


def eot_text(n, length, e, gen):
    t = normal_tokens(n, length, e, gen)
    eot = torch.randint(8, length, (n,), device=dev, generator=gen)
    tail = t[torch.arange(n, device=dev), eot]
    mask = torch.arange(length, device=dev).unsqueeze(0) >= eot.unsqueeze(1)
    t[mask] = tail.unsqueeze(1).expand(n, length, e)[mask]
    return t


def stage_one(index, qf, C):
    """the first stage of search(candidates=C), as search.py runs it -> (values, positions)"""
    nq = qf.shape[0]
    val, idx = ops.topk_init(nq, C, dev)
    image = index.kind == "image"
    step = min(index.QUERY_CHUNK, nq)
    for q0 in range(0, nq, step):
        for base, gf, _ in index.chunks():
            G = similarity_matrix(gf, qf[q0:q0 + step]) if image else similarity_matrix(qf[q0:q0 + step], gf)
            ops.topk_merge(G, 1 if image else 0, base, val[q0:q0 + step], idx[q0:q0 + step])
    return val, idx


def measure(index, qf, qt, iters, label):
    found = {}

    def arm(C):
        def run():
            found[C] = index.search(qf, qt, K, candidates=C)
        return run

    arms = {"exhaustive": arm(None)}
    arms.update({f"C={C}": arm(C) for C in CS})
    t = alternate(arms, iters)
    base = statistics.median(t["exhaustive"])
    print(f"  {label}: {line('exhaustive search', t['exhaustive'])}", flush=True)
    ids0 = found[None][1]
    for C in CS:
        tc = t[f"C={C}"]
        cand = {}

        def s1():
            cand["c"] = stage_one(index, qf, C)

        def s2():
            index.rerank(qf, qt, cand["c"][1], K, global_scores=cand["c"][0])

        s1()
        ts = alternate({"stage 1": s1, "stage 2": s2}, max(3, iters // 4))
        ids = found[C][1]
        kept = (ids0.unsqueeze(2) == ids.unsqueeze(1)).any(2).float().mean(1)
        top1 = float((ids0[:, 0] == ids[:, 0]).float().mean())
        print(f"    candidates={C}: {line('search', tc)} = {base / statistics.median(tc):.2f}x the exhaustive one | "
              f"{line('stage 1 (global GEMM + top-C)', ts['stage 1'])} | {line('stage 2 (rerank)', ts['stage 2'])} | of the exhaustive "
              f"top-10 returned: mean {float(kept.mean()):.4f}, same top-1 {100 * top1:.2f} % (random unit features, global and token "
              f"similarities independent: understates a trained model)", flush=True)


gen = torch.Generator(device=dev).manual_seed(0)
NI, NT, Q, N, E = 5000, 25000, 49, 77, 512
print(f"b. {NI} images x {NT} captions, q = {Q}, n = {N}, E = {E}, bf16, EOT-shaped text, k = {K}, {args.iters} alternating iterations",
      flush=True)
fi = torch.nn.functional.normalize(torch.randn(NI, E, device=dev, generator=gen), dim=-1)
ft = torch.nn.functional.normalize(torch.randn(NT, E, device=dev, generator=gen), dim=-1)
ti = normal_tokens(NI, Q, E, gen)
tt = eot_text(NT, N, E, gen)
for kind in ("image", "text"):
    index = LateInteractionIndex(kind, alpha=0.5, scale=14.0, device=dev)
    index.add(fi, ti) if kind == "image" else index.add(ft, tt)
    qf, qt = (ft, tt) if kind == "image" else (fi, ti)
    measure(index, qf, qt, args.iters, f"{'text' if kind == 'image' else 'image'} queries over the {kind}s")
    del index
del fi, ft, ti, tt
torch.cuda.empty_cache()

if not args.skip_large:
    NG, NQ = 200000, 2000
    print(f"c. {NG} images x {NQ} text queries, same token shapes, k = {K}", flush=True)
    qf = torch.nn.functional.normalize(torch.randn(NQ, E, device=dev, generator=gen), dim=-1)
    qt = eot_text(NQ, N, E, gen)
    index = LateInteractionIndex("image", alpha=0.5, scale=14.0, device=dev)
    for lo in range(0, NG, 20000):
        index.add(torch.nn.functional.normalize(torch.randn(20000, E, device=dev, generator=gen), dim=-1), normal_tokens(20000, Q, E, gen))
    measure(index, qf, qt, max(3, args.iters // 5), "text queries over the images")
