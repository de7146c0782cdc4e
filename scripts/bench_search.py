"""Time late-interaction search (colxlip_amd/search.py, csrc/topk.hip) against the dense route (the whole score matrix, then
torch.topk).  All arms of a measurement ALTERNATE inside this process, every shape is warmed up first, each arm reports its
median and min .. max.

  a. the merge kernel alone on one COCO-shaped tile (5 000 images x 25 000 captions, image-major fp32): 25 000 text queries over
     5 000 candidates (lane per query) and 5 000 image queries over 25 000 candidates (wave per query), k = 10 and 100, against
     torch.topk of the tile + torch.cat with a running list + torch.topk.  Bytes/s on the 4 * nq * nc bytes the kernel must read,
     as a share of the 6.3 TB/s streaming rate of the MI355X.
  b. end to end at 5 000 images x 25 000 captions, ViT-B/32-colxlip token shapes (q = 49, n = 77, E = 512, bf16, EOT-shaped text):
     LateInteractionIndex.search against ops.maxsim_scores into the dense matrix + torch.topk, both directions, k = 10; and a
     third arm, the same search over an index with token_dtype="fp8" (e4m3 tokens, MaxSim GEMM on the fp8 MFMA), with the index
     bytes per item, the cost of quantising the queries alone, and how far the results move: the share of each query's bf16
     top-10 that the fp8 top-10 keeps and the largest |score difference| over the slots where the ids agree.
  c. a gallery the dense route would need 1.6 GB of scores for: 200 000 images x 2 000 text queries: time and peak memory, for
     the default index and the fp8 one.

    python scripts/bench_search.py [--iters 10] [--skip-large]"""
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
ap.add_argument("--iters", type=int, default=10)
ap.add_argument("--skip-large", action="store_true")
args = ap.parse_args()
assert torch.cuda.is_available(), "bench_search.py measures on the GPU"
dev = "cuda"
STREAM = 6.3e12                                    # bytes/s a streaming read achieves on the MI355X


def one(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def alternate(arms, iters, before=None):
    """{name: [ms]}: two warm-up calls per arm, then the arms alternate iteration by iteration; `before` runs untimed before
    every call"""
    times = {name: [] for name in arms}
    for fn in arms.values():
        for _ in range(2):
            if before:
                before()
            fn()
    torch.cuda.synchronize()
    for _ in range(iters):
        for name, fn in arms.items():
            if before:
                before()
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


gen = torch.Generator(device=dev).manual_seed(0)
NI, NT, Q, N, E = 5000, 25000, 49, 77, 512

# ---------------------------------------------------------------------------------------------------- a. the kernel alone
print("a. clipx_topk_merge on one tile [5000 images, 25000 captions] fp32 (500 MB), lists empty before every call", flush=True)
tile = torch.randn(NI, NT, device=dev, generator=gen)
for query_dim, nq, nc in ((1, NT, NI), (0, NI, NT)):
    for k in (10, 100):
        state = {}

        def fresh():
            state["best"] = ops.topk_init(nq, k, dev)
            state["run_v"] = torch.full((nq, k), float("-inf"), device=dev)
            state["run_i"] = torch.full((nq, k), -1, dtype=torch.int64, device=dev)

        def merge():
            ops.topk_merge(tile, query_dim, 0, *state["best"])

        def torch_route():
            v, i = torch.topk(tile, min(k, nc), dim=1 - query_dim)
            if query_dim == 1:
                v, i = v.t(), i.t()
            v2, j = torch.topk(torch.cat([state["run_v"], v], dim=1), k, dim=1)
            state["out"] = (v2, torch.cat([state["run_i"], i], dim=1).gather(1, j))

        t = alternate({"merge": merge, "torch": torch_route}, args.iters, before=fresh)
        fresh()
        merge()
        torch_route()
        same = bool(torch.equal(state["best"][0], state["out"][0]))
        rate = 4.0 * nq * nc / (statistics.median(t["merge"]) * 1e-3)
        print(f"  {nq} queries x {nc} candidates ({'lane' if query_dim == 1 else 'wave'} per query), k = {k}: {line('merge', t['merge'])} = "
              f"{rate / 1e12:.2f} TB/s = {100 * rate / STREAM:.0f} % of streaming | {line('torch.topk + cat + topk', t['torch'])} | "
              f"values equal: {same}", flush=True)
del tile
torch.cuda.empty_cache()

# ---------------------------------------------------------------------------------------------------- b. end to end
print(f"b. end to end, {NI} images x {NT} captions, q = {Q}, n = {N}, E = {E}, bf16, EOT-shaped text, k = 10", flush=True)
fi = torch.nn.functional.normalize(torch.randn(NI, E, device=dev, generator=gen), dim=-1)
ft = torch.nn.functional.normalize(torch.randn(NT, E, device=dev, generator=gen), dim=-1)
ti = normal_tokens(NI, Q, E, gen)
tt = eot_text(NT, N, E, gen)
for kind in ("image", "text"):
    index = LateInteractionIndex(kind, alpha=0.5, scale=14.0, device=dev)
    qf, qt = (ft, tt) if kind == "image" else (fi, ti)
    index.add(fi, ti) if kind == "image" else index.add(ft, tt)
    index8 = LateInteractionIndex(kind, alpha=0.5, scale=14.0, device=dev, token_dtype="fp8")
    index8.add(fi, ti) if kind == "image" else index8.add(ft, tt)
    found = {}

    def stream():
        found["stream"] = index.search(qf, qt, 10)

    def dense():
        scores = ops.maxsim_scores(ti, tt, similarity_matrix(fi, ft), 0.5, 14.0)
        v, i = torch.topk(scores, 10, dim=0 if kind == "image" else 1)
        found["dense"] = (v.t(), i.t()) if kind == "image" else (v, i)

    def stream8():
        found["fp8"] = index8.search(qf, qt, 10)

    def quantise_queries():                                      # what search() does to the query tokens, per query chunk, alone
        step = LateInteractionIndex.QUERY_CHUNK
        for q0 in range(0, qt.shape[0], step):
            part = qt[q0:q0 + step]
            ops.quant_tokens_e4m3(part)
            if kind == "image":
                ops.maxsim_text_counts(part)

    t = alternate({"stream": stream, "dense": dense, "fp8": stream8, "quantise": quantise_queries}, args.iters)
    ms, md = statistics.median(t["stream"]), statistics.median(t["dense"])
    spread = max(t["dense"]) - min(t["dense"])
    agree = float((found["stream"][1] == found["dense"][1]).float().mean())
    print(f"  {'text' if kind == 'image' else 'image'} queries over the {kind}s: {line('LateInteractionIndex.search', t['stream'])} | "
          f"{line('maxsim_scores + torch.topk', t['dense'])} | stream - dense = {ms - md:+.3f} ms, the baseline's own spread "
          f"{spread:.3f} ms: within the bar: {'yes' if ms - md <= spread else 'NO'} | ids agree on {100 * agree:.2f} % of slots", flush=True)
    m8, mq = statistics.median(t["fp8"]), statistics.median(t["quantise"])
    items = len(index)
    per16, per8 = index.token_bytes() / items, index8.token_bytes() / items
    print(f"    token_dtype=fp8: {line('LateInteractionIndex.search', t['fp8'])} = {ms / m8:.2f}x the bf16 index | "
          f"{line('quantising the queries alone', t['quantise'])} = {100 * mq / m8:.1f} % of it", flush=True)
    print(f"    index bytes per item: tokens {per16:.0f} (bf16) -> {per8:.0f} (e4m3 + exponents{' + counts' if kind == 'text' else ''}) = "
          f"{per8 / per16:.4f}; + {4 * E} of fp32 global features and 8 of id either way", flush=True)
    ids16, ids8 = found["stream"][1], found["fp8"][1]
    kept = (ids16.unsqueeze(2) == ids8.unsqueeze(1)).any(2).float().mean(1)                     # per query: share of the bf16 top-10
    same = ids16 == ids8
    diff = float((found["stream"][0] - found["fp8"][0])[same].abs().max()) if bool(same.any()) else float("nan")
    top1 = float(same[:, 0].float().mean())
    print(f"    fp8 against bf16 results (random unit features: neighbouring scores lie closer than a trained model's): top-10 kept "
          f"mean {float(kept.mean()):.4f} min {float(kept.min()):.2f} | same top-1 {100 * top1:.2f} % | max |score difference| where "
          f"the ids agree {diff:.3e} (scores {float(found['stream'][0].min()):.2f} .. {float(found['stream'][0].max()):.2f})", flush=True)
    del index, index8
del fi, ft, ti, tt
torch.cuda.empty_cache()

# ---------------------------------------------------------------------------------------------------- c. a large gallery
if not args.skip_large:
    NG, NQ = 200000, 2000
    print(f"c. {NG} images x {NQ} text queries, same token shapes, k = 10 (dense scores alone: {NG * NQ * 4 / 1e9:.1f} GB)", flush=True)
    qf = torch.nn.functional.normalize(torch.randn(NQ, E, device=dev, generator=gen), dim=-1)
    qt = eot_text(NQ, N, E, gen)
    for token_dtype in (None, "fp8"):
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated()
        index = LateInteractionIndex("image", alpha=0.5, scale=14.0, device=dev, token_dtype=token_dtype)
        for lo in range(0, NG, 20000):
            index.add(torch.nn.functional.normalize(torch.randn(20000, E, device=dev, generator=gen), dim=-1), normal_tokens(20000, Q, E, gen))
        index.search(qf[:64], qt[:64], 10)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        live = torch.cuda.memory_allocated()
        times = [one(lambda: index.search(qf, qt, 10)) for _ in range(3)]
        peak = torch.cuda.max_memory_allocated() - live
        print(f"  token_dtype={token_dtype}: gallery on the device {(live - before) / 1e9:.2f} GB | {line('search', times)} (first call "
              f"included) | peak above live memory {peak / 1e6:.1f} MB", flush=True)
        del index
        torch.cuda.empty_cache()
