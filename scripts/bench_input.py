"""Time the real-image input path on one GPU (`--dataset-type packed`: data.PackedLoader + ops.image_transform) and what it costs
the train step.  Three measurements, from a generated packed set of `--images` noise images whose shortest side is 256 px
(longest 256..384), read back through the page cache:

  loader    images/s of PackedLoader alone at 224 px (gather on `--workers` threads, copy, kernel), batches dropped as they come
  stages    per batch of `--batch`: host gather ms (wall clock), host-to-device copy ms and transform kernel ms (device events)
  step      ViT-B/32, bf16, batch `--batch`: ms/step of the full train step fed by SyntheticLoader and fed by PackedLoader, in
            alternating rounds in this one process

    python scripts/bench_input.py [--images 8192] [--batch 4096] [--workers 16] [--steps 6] [--rounds 3] [--out FILE]

Step and loader times are host clocks around work that ends in a device synchronise; copy and kernel times are device events.
`--generate-only DIR` writes the packed set and stops (no GPU needed)."""
import argparse
import json
import math
import os
import shutil
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from colxlip_amd import create_model_and_transforms, ops  # noqa: E402
from colxlip_amd.data import PackedDataset, PackedLoader, SyntheticLoader, synthetic_batch  # noqa: E402
from colxlip_amd.image_transform import transform_from  # noqa: E402
from colxlip_amd.loss import ClipLoss  # noqa: E402
from colxlip_amd.optim import FusedAdamW, param_groups  # noqa: E402
from colxlip_amd.pack import write_packed  # noqa: E402


def generate(root, n, seed=0):
    """n uint8 noise images, shortest side 256, longest 256..384, either orientation; one caption each, its token ids drawn by
    the synthetic loader's recipe (`data.synthetic_batch`: EOT uniform in [8, L-1]) so that the text tower sees the same lengths
    whichever loader feeds the step"""
    rng = np.random.default_rng(seed)
    noise = rng.integers(0, 256, 1 << 24, dtype=np.uint8)

    def images():
        for i in range(n):
            long_side = int(rng.integers(256, 385))
            h, w = (256, long_side) if i % 2 else (long_side, 256)
            start = int(rng.integers(0, noise.size - 3 * h * w))
            yield noise[start:start + 3 * h * w].reshape(h, w, 3)

    captions = [[str(i)] for i in range(n)]

    def tokens(texts, context_length=77):
        return synthetic_batch(len(texts), 8, context_length, 49408, seed=seed + 1)[1][:, 0]

    tokens.vocab_size = 49408
    return write_packed(root, images(), captions, tokens, tokenizer_name="synthetic ids")


def emit(out, row):
    line = json.dumps(row)
    print(line, flush=True)
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")


def endless(loader):
    epoch = 0
    while True:
        if hasattr(loader, "set_epoch"):
            loader.set_epoch(epoch)
        yield from loader
        epoch += 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=8192)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--workers", type=int, default=16)
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--model", default="ViT-B-32")
    ap.add_argument("--out", default=None)
    ap.add_argument("--generate-only", default=None, metavar="DIR")
    a = ap.parse_args()
    if a.generate_only:
        print(json.dumps(generate(a.generate_only, a.images)))
        return
    assert torch.cuda.is_available(), "bench_input.py measures on the GPU"
    dev = "cuda:0"
    root = tempfile.mkdtemp(prefix="packed_bench_")
    try:
        t0 = time.perf_counter()
        meta = generate(root, a.images)
        ds = PackedDataset(root)
        emit(a.out, {"what": "dataset", "images": meta["n"], "bytes": int(ds.images.size), "generate_s": round(time.perf_counter() - t0, 1)})

        torch.manual_seed(0)
        model, pre_train, _ = create_model_and_transforms(a.model, precision="bf16", device=dev, output_dict=True)
        model.train()
        transform = transform_from(pre_train, True, None, model.visual.image_size)
        packed = PackedLoader(ds, a.batch, transform, dev, image_dtype=torch.bfloat16, workers=a.workers)
        per_epoch = packed.num_batches

        # ---- loader alone
        feed = endless(packed)
        for _ in range(per_epoch):
            next(feed)
        torch.cuda.synchronize()
        n_b = max(a.steps, per_epoch)
        t0 = time.perf_counter()
        for _ in range(n_b):
            next(feed)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        feed.close()
        emit(a.out, {"what": "loader", "size": list(transform.size), "batch": a.batch, "workers": a.workers, "batches": n_b,
                     "ms_per_batch": round(1e3 * dt / n_b, 2), "images_per_s": round(n_b * a.batch / dt, 1)})

        # ---- stages of one batch: gather (host), copy, kernel (device events)
        stream = packed._stream
        idx, gen = packed.plan(0)[0]
        gather_ms, copy_ms, kernel_ms = [], [], []
        for rep in range(4):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            st = stream._start(rep, idx, packed.batch_generator(0, 0))
            for f in st.futures:
                f.result()
            gather_ms.append(1e3 * (time.perf_counter() - t0))
            stage = stream._stage[st.slot]
            raw = torch.empty(st.total, dtype=torch.uint8, device=dev)
            e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
            e[0].record()
            raw.copy_(stage[:st.total], non_blocking=True)
            e[1].record()
            images = transform(raw[st.img_off:st.total], raw[:48 * st.n].view(torch.int64).view(st.n, 6), torch.bfloat16)
            e[2].record()
            torch.cuda.synchronize()
            copy_ms.append(e[0].elapsed_time(e[1]))
            kernel_ms.append(e[1].elapsed_time(e[2]))
        moved = st.total + images.numel() * 2
        emit(a.out, {"what": "stages", "batch": a.batch, "staged_bytes": int(st.total), "gather_ms": [round(v, 2) for v in gather_ms],
                     "copy_ms": [round(v, 2) for v in copy_ms], "kernel_ms": [round(v, 3) for v in kernel_ms],
                     "kernel_GBps_min_time": round(moved / (min(kernel_ms) * 1e6), 1)})
        del raw, images

        # ---- the train step, fed by each loader in alternating rounds
        synthetic = SyntheticLoader(a.batch, a.batch * per_epoch, model.visual.image_size, model.context_length, model.vocab_size,
                                    dev, image_dtype=torch.bfloat16)
        loss_fn = ClipLoss(cache_labels=True)
        opt = FusedAdamW(param_groups(model.named_parameters(), 0.2), lr=1e-6, betas=(0.9, 0.98), eps=1e-6)

        def run(feed, steps):
            for _ in range(steps):
                images, texts = next(feed)
                opt.zero_grad(set_to_none=True)
                out = model(images, texts[:, 0].contiguous())
                loss_fn(**out).backward()
                opt.step()
                ops.clamp1(model.logit_scale.data, 0.0, math.log(100))

        feeds = {"synthetic": endless(synthetic), "packed": endless(packed)}
        for name, feed in feeds.items():
            run(feed, 2)
        torch.cuda.synchronize()
        times = {name: [] for name in feeds}
        for _ in range(a.rounds):
            for name, feed in feeds.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                run(feed, a.steps)
                torch.cuda.synchronize()
                times[name].append(1e3 * (time.perf_counter() - t0) / a.steps)
        feeds["packed"].close()
        row = {"what": "step", "model": a.model, "precision": "bf16", "batch": a.batch, "steps_per_round": a.steps}
        for name, ts in times.items():
            row[name + "_ms_per_step"] = [round(t, 2) for t in ts]
            row[name + "_images_per_s_median"] = round(a.batch / (float(np.median(ts)) * 1e-3), 1)
        row["packed_over_synthetic_median"] = round(float(np.median(times["packed"]) / np.median(times["synthetic"])), 4)
        emit(a.out, row)
    finally:
        shutil.rmtree(root, ignore_errors=True)


if __name__ == "__main__":
    main()
