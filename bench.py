"""Headline benchmark: images/sec of the full CLIP train step (zero_grad -> image+text towers fwd ->
ClipLoss -> bwd -> gradient sync -> fused AdamW -> logit_scale clamp) for ViT-B/32 + 77-token text
at GLOBAL batch 4096 (BASELINE.json), bf16 operands / fp32 accumulate, synthetic data, random init.

    python bench.py                                   # 1 GPU, defaults finish within minutes
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
           --master-port P bench.py --gpus N --steps K --warmup W

Prints ONE JSON line on rank 0 (contract in the task statement).  A plain run sets up, warms up, times the K steps, writes
--dump-outputs if asked and prints that line: nothing else.  --full adds, after the timed region, what needs runs of its own:
  dense_text_rows — a short second measurement of the same step with all 77 text positions computed (--no-dense-compare: off).
  roofline        — the dominant kernel (bf16 MFMA NT GEMM: every forward linear and every dgrad),
                    algorithmic FLOPs of its launches / their measured durations (HIP events recorded on the
                    launch stream around each launch, in an instrumented step after the timed region).
  cpu_baseline    — the CPU oracle (a port of the reference's PyTorch path) timed on the host cores on a
                    bounded sample (ViT-B/32, batch 32, fp32 full train steps), rank 0 at N=1 only (--no-cpu-baseline: off).

--dump-outputs DIR writes what the last timed step computed on rank 0 as DIR/<name>.npy (float32): `loss`, every tensor of the
model's output dict, and `param.<name>` / `grad.<name>` for every parameter after the optimizer step.  Inputs and init are seeded,
so two builds run with the same arguments can be compared array for array.
"""
import argparse
import json
import math
import os
import sys
import time

# multi-process GPU work on this pool needs dmabuf IPC (the host driver has no legacy IPC): already exported on the boxes, set here
# as well so that a launcher with a scrubbed environment does not turn RCCL's first collective into hipIpcGetMemHandle errors
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")

import torch  # noqa: E402

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

PEAK_BF16_DENSE_TFLOPS = 2500.0      # MI355X_MICROARCH.md: ~2.5 PF dense bf16 MFMA
PEAK_FP8_DENSE_TFLOPS = 5000.0       # MI355X_MICROARCH.md: ~5 PF dense fp8 MFMA
FWD_BWD_GFLOP_PER_PAIR = {"ViT-B-32": 44.3, "ViT-B-16": 123.3, "ViT-L-14-336": 1185.7, "ViT-H-14": 1145.0}
DUMP_LIMIT_BYTES = 64 << 20
DUMP_OUTPUT_ELEMS = 1 << 21          # a model output up to this size is written whole (ViT-B/32 at batch 4096: 4096 x 512)
DUMP_PARAM_ELEMS = 4096              # per parameter and per gradient


def parse():
    p = argparse.ArgumentParser()
    p.add_argument("--gpus", type=int, default=1)
    p.add_argument("--steps", type=int, default=8)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--model", default="ViT-B-32")
    p.add_argument("--global-batch", type=int, default=4096)
    p.add_argument("--precision", default="bf16")
    p.add_argument("--grad-checkpointing", action="store_true")
    p.add_argument("--full", action="store_true",
                   help="after the timed region also measure the dense text layout, run the instrumented step behind `roofline` "
                        "and time the CPU baseline (a plain run does only what `value` and --dump-outputs need)")
    p.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline")
    p.add_argument("--cpu-steps", type=int, default=15, help="with --full: timed CPU baseline steps at most")
    p.add_argument("--serial-towers", action="store_true",
                   help="run the two towers on one stream (per-kernel durations in a rocprofv3 trace are only meaningful "
                        "when kernels do not overlap; the default overlaps them and is what `value` reports)")
    p.add_argument("--dense-text", action="store_true",
                   help="compute all 77 text positions like the reference (default: only positions 0..EOT, packed rows)")
    p.add_argument("--no-dense-compare", action="store_true",
                   help="with --full: skip the short second measurement with the dense text layout that is reported beside `value`")
    p.add_argument("--force-dist", action="store_true",
                   help="1-GPU rehearsal of the multi-GPU path: RCCL process group of one rank, gradient all-reduce on")
    p.add_argument("--shard-optimizer", action="store_true",
                   help="ZeRO-1 (reduce-scatter the gradient arenas, AdamW on each rank's slices, all-gather the parameters): "
                        "off by default until it has been measured on more than one GPU")
    p.add_argument("--colclip-global", action="store_true",
                   help="ColXLIP models at N > 1: the reference's global token logits on every rank instead of each rank's own rows")
    p.add_argument("--rehearse-on-one-gpu", action="store_true",
                   help="N > 1 ranks that SHARE device 0 over gloo (RCCL refuses two ranks on one device): runs the exact N > 1 "
                        "bench path -- per-rank batch shard, feature gather in the loss, gradient hooks -- on a one-GPU box "
                        "(tests/test_two_ranks_gpu.py); its timings mean nothing")
    p.add_argument("--dump-outputs", metavar="DIR",
                   help="write the outputs of the last timed step as DIR/<name>.npy (rank 0), for comparing two builds")
    a = p.parse_args()
    if a.steps < 1 or a.warmup < 0:
        p.error("--steps must be at least 1 and --warmup at least 0")
    return a


class LaunchTimer:
    """HIP events on the current stream around selected launches (instrumented step only)."""

    def __init__(self):
        self.records = []

    def wrap(self, fn, flops_of, bytes_of):
        def inner(*a, **k):
            e0 = torch.cuda.Event(enable_timing=True)
            e1 = torch.cuda.Event(enable_timing=True)
            e0.record()
            r = fn(*a, **k)
            e1.record()
            self.records.append((e0, e1, flops_of(*a, **k), bytes_of(*a, **k)))
            return r
        return inner

    def totals(self):
        torch.cuda.synchronize()
        ms = sum(e0.elapsed_time(e1) for e0, e1, _, _ in self.records)
        fl = sum(f for _, _, f, _ in self.records)
        by = sum(b for _, _, _, b in self.records)
        return len(self.records), ms, fl, by


def _fwd_bytes(x, w, bias=None, act=0, want_preact=False, residual=None, out_dtype=None, out=None):
    """Algorithmic HBM bytes of one forward linear: each operand read once, each result written once."""
    M, K = x.shape
    N = w.shape[0]
    osz = 4 if (out_dtype == torch.float32 or (out is not None and out.dtype == torch.float32)) else x.element_size()
    return x.element_size() * (M * K + N * K) + osz * M * N + ((1 if want_preact == "gelu8" else x.element_size()) * M * N if want_preact else 0) + \
        (x.element_size() * M * N if residual is not None else 0) + (4 * N if bias is not None else 0)


def _fwd8_bytes(x8, xe, w8, we, bias=None, act=0, want_preact=False, residual=None, out=None):
    """fp8 forward linear: e4m3 operands (1 B/element) + one int32 exponent per row, bf16 results / epilogue operands."""
    M, K = x8.shape
    N = w8.shape[0]
    return M * K + N * K + 4 * (M + N) + 2 * M * N * (1 + (1 if want_preact else 0) + (1 if residual is not None else 0)) + \
        (4 * N if bias is not None else 0)


def _dgrad8_bytes(dy8, dye, wt8, wte, act=0, u=None, out=None):
    M, N = dy8.shape
    K = wt8.shape[0]
    return M * N + N * K + 4 * (M + K) + 2 * M * K * (1 + (1 if u is not None else 0))


def _dgrad_bytes(dy, w, wt, act=0, u=None, out=None):
    M, N = dy.shape
    K = w.shape[1] if w is not None else wt.shape[0]
    return dy.element_size() * (M * N + N * K + M * K) + (u.element_size() * M * K if u is not None else 0)


NT_KERNEL_SOURCES = ("gemm_bf16_nt.hip", "gemm_bf16_nt8p.hip", "gemm_bf16_nt5.hip", "gemm_nt5_acc.inc", "gemm_epi.h",
                     "gemm_nt_epilogue.h", "linear.hip")


def nt_kernel_rev():
    """sha256 over the CODE of the dominant kernel's sources (comments and white space stripped, so that editing a comment does
    not orphan a measurement): a PMC measurement is only valid for the code it was taken on."""
    import hashlib
    import re
    h = hashlib.sha256()
    for name in NT_KERNEL_SOURCES:
        with open(os.path.join(ROOT, "colxlip_amd", "csrc", name), "r") as f:
            src = f.read()
        src = re.sub(r"/\*.*?\*/", " ", src, flags=re.S)
        src = re.sub(r"//[^\n]*", " ", src)
        h.update(" ".join(src.split()).encode())
    return h.hexdigest()[:16]


def pmc_traffic(model, per_gpu_batch, precision, text_rows):
    """HBM bytes per launch of the dominant kernel from the committed PMC passes (profiles/pmc_traffic.json:
    separate rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE runs of this same command, gfx950-corrected; scripts/pmc_summary.py
    writes the entry).  Counters cannot be read from inside the process, so this is the last committed measurement --
    used only when it was taken on the SAME kernel sources (kernel_rev) and workload, else None."""
    try:
        with open(os.path.join(ROOT, "profiles", "pmc_traffic.json")) as f:
            table = json.load(f)
    except OSError:
        return None
    rec = table.get(f"{model}/b{per_gpu_batch}/{precision}/{text_rows}")
    if not rec or rec.get("kernel_rev") != nt_kernel_rev():
        return None
    return rec["traffic_bytes_per_launch"]


def host_cores():
    """Threads the CPU baseline uses: the PHYSICAL cores (one thread per core: SMT siblings add nothing to fp32 GEMMs) inside
    this process's scheduler affinity, capped by the cgroup CPU quota when one is set (asking OpenMP for more threads than the
    quota grants makes the baseline crawl: 100+ spinning threads on a 16-CPU quota).  CLIPX_CPU_THREADS overrides."""
    forced = os.environ.get("CLIPX_CPU_THREADS")
    if forced and forced.isdigit() and int(forced) > 0:
        return int(forced)
    try:
        allowed = set(os.sched_getaffinity(0))
    except AttributeError:
        allowed = set(range(os.cpu_count() or 1))
    n = len(allowed)
    try:        # distinct (socket, core) pairs among the allowed logical CPUs
        cores, cpu, phys = set(), None, None
        with open("/proc/cpuinfo") as f:
            for line in f:
                key, _, val = line.partition(":")
                key = key.strip()
                if key == "processor":
                    cpu, phys = int(val), None
                elif key == "physical id":
                    phys = val.strip()
                elif key == "core id" and cpu in allowed:
                    cores.add((phys, val.strip()))
        if cores:
            n = min(n, len(cores))
    except (OSError, ValueError):
        pass
    for path in ("/sys/fs/cgroup/cpu.max", "/sys/fs/cgroup/cpu/cpu.cfs_quota_us"):
        try:
            with open(path) as f:
                parts = f.read().split()
            if path.endswith("cpu.max"):
                if parts[0] != "max":
                    n = min(n, max(1, int(int(parts[0]) / int(parts[1]))))
            else:
                q = int(parts[0])
                if q > 0:
                    with open("/sys/fs/cgroup/cpu/cpu.cfs_period_us") as f:
                        n = min(n, max(1, q // int(f.read().split()[0])))
            break
        except (OSError, ValueError, IndexError):
            continue
    return max(1, n)


def _flat_sample(t, k):
    """`t` as float32 on the host; above k elements a fixed, seeded sample of k of them, flattened (the indices depend only on
    t.numel(), so the same sample is taken from every build)."""
    t = t.detach()
    if t.numel() > k:
        idx = torch.randint(0, t.numel(), (k,), generator=torch.Generator().manual_seed(0)).sort().values
        t = t.reshape(-1)[idx.to(t.device)]
    return t.float().cpu().numpy()


def dump_outputs(path, loss, out, model):
    """What a caller of the train step holds after it: the loss, the model's outputs, the updated parameters and their gradients."""
    import numpy as np
    arrays = {"loss": _flat_sample(loss, 1)}
    arrays.update({k: _flat_sample(v, DUMP_OUTPUT_ELEMS) for k, v in out.items() if isinstance(v, torch.Tensor)})
    for name, p in model.named_parameters():
        arrays["param." + name] = _flat_sample(p, DUMP_PARAM_ELEMS)
        if p.grad is not None:
            arrays["grad." + name] = _flat_sample(p.grad, DUMP_PARAM_ELEMS)
    total = sum(a.nbytes for a in arrays.values())
    assert total <= DUMP_LIMIT_BYTES, f"--dump-outputs: {total} bytes exceed {DUMP_LIMIT_BYTES}"
    os.makedirs(path, exist_ok=True)
    for name, a in arrays.items():
        np.save(os.path.join(path, name + ".npy"), a)
    print(f"[bench] wrote {len(arrays)} arrays ({total / 2**20:.1f} MiB) to {path}", file=sys.stderr, flush=True)


def cpu_model():
    try:
        with open("/proc/cpuinfo") as f:
            for line in f:
                if line.startswith("model name"):
                    return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def cpu_baseline(steps, budget_s=25.0):
    """Oracle (CPU port of the reference path): ViT-B/32, batch 32, fp32, full train steps; bounded in time."""
    from oracle import clip_oracle as O
    cores = host_cores()
    torch.set_num_threads(cores)
    cfg = O.VIT_B_32
    sd = O.init_state_dict(cfg, seed=0)
    batch = 32
    params = {k: v.clone() for k, v in sd.items()}
    m = {k: torch.zeros_like(v) for k, v in params.items()}
    v = {k: torch.zeros_like(v) for k, v in params.items()}
    image, text = O.synthetic_batch(cfg, batch, seed=1234)

    def one(step):
        _, _, grads = O.loss_and_grads(params, image, text, cfg)
        O.adamw_step(params, grads, m, v, step)

    t0 = time.time()
    one(1)
    print(f"[bench] cpu_baseline warm-up step {time.time() - t0:.1f}s on {cores} threads", file=sys.stderr, flush=True)
    done, t0 = 0, time.time()
    while done < steps and (done == 0 or time.time() - t0 < budget_s):
        one(2 + done)
        done += 1
        print(f"[bench] cpu_baseline step {done} at {time.time() - t0:.1f}s", file=sys.stderr, flush=True)
    dt = (time.time() - t0) / done
    return {"value": round(batch / dt, 2), "unit": "images/sec", "cores": cores, "cpu": cpu_model(), "kind": "port",
            "sample": f"ViT-B/32 + text tower, batch {batch}, fp32, 1 warm-up + {done} timed full train steps "
                      f"(fwd+loss+bwd+AdamW) of oracle/clip_oracle.py on {cores} host threads"}


def main():
    args = parse()
    rank = int(os.environ.get("RANK", 0))
    local_rank = int(os.environ.get("LOCAL_RANK", 0))
    world = int(os.environ.get("WORLD_SIZE", 1))
    assert world == args.gpus, f"--gpus {args.gpus} but WORLD_SIZE={world}"
    if args.rehearse_on_one_gpu:
        local_rank = 0
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    if world > 1 or args.force_dist:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29533")
        # RCCL writes its version banner to STDOUT when the communicator is created; stdout must carry the one JSON line only,
        # so file descriptor 1 points at stderr while the process group and its first collective are set up
        sys.stdout.flush()
        saved = os.dup(1)
        os.dup2(2, 1)
        try:
            if args.rehearse_on_one_gpu:
                torch.distributed.init_process_group("gloo", rank=rank, world_size=world)
            else:
                torch.distributed.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
            torch.distributed.barrier()
            torch.cuda.synchronize()
        finally:
            sys.stdout.flush()
            os.dup2(saved, 1)
            os.close(saved)

    if args.serial_towers:
        os.environ["CLIPX_TOWER_STREAMS"] = "0"
    if args.dense_text:
        os.environ["CLIPX_TEXT_UNPAD"] = "0"
    import colxlip_amd
    from colxlip_amd import create_model_and_transforms, ops
    from colxlip_amd.data import synthetic_batch
    from colxlip_amd.distributed import GradSync
    from colxlip_amd.loss import ClipLoss
    from colxlip_amd.optim import FusedAdamW, param_groups
    from colxlip_amd.scheduler import cosine_lr

    assert args.global_batch % world == 0
    b = args.global_batch // world
    torch.manual_seed(0)                      # same init on every rank (reference main.py:220)
    model, _, _ = create_model_and_transforms(args.model, precision=args.precision, device=dev, output_dict=True)
    if args.grad_checkpointing:
        model.set_grad_checkpointing(True)
    model.train()
    colxlip = "colxlip" in args.model.lower()
    if colxlip:
        # the fork's own model + loss (reference factory.py:286-287,443-452; launch point src/colxlip.sh:38,52: global logits on
        # every rank, loss.py:246-256 refuses local_loss): token features gathered like the pooled ones
        from colxlip_amd.loss import ColClipLoss
        # N > 1: each rank computes its own text rows of the token logits (`rows_local`, an extension: same mean loss and
        # gradients as the reference's global logits on every rank, 1/W of the MaxSim work); --colclip-global = the reference's form
        loss_fn = ColClipLoss(local_loss=False, gather_with_grad=world > 1, cache_labels=True, rank=rank, world_size=world, alpha=0.5,
                              rows_local=(world > 1 and not args.colclip_global))
    else:
        loss_fn = ClipLoss(local_loss=world > 1, gather_with_grad=world > 1, cache_labels=True, rank=rank, world_size=world)
    shard = args.shard_optimizer and (world > 1 or args.force_dist)
    sync = GradSync(list(model.parameters()), world, force=args.force_dist, shard_optimizer=shard).attach(model)
    if shard:
        from colxlip_amd.optim import ShardedAdamW
        opt = ShardedAdamW(param_groups(model.named_parameters(), 0.2), sync, lr=5e-4, betas=(0.9, 0.98), eps=1e-6)
    else:
        opt = FusedAdamW(param_groups(model.named_parameters(), 0.2), lr=5e-4, betas=(0.9, 0.98), eps=1e-6)
    image_size = model.visual.image_size
    images, texts = synthetic_batch(b, image_size, model.context_length, model.vocab_size, seed=1234 + rank, device=dev,
                                    image_dtype=torch.bfloat16 if args.precision != "fp32" else torch.float32)
    texts = texts[:, 0].contiguous()
    # lr 5e-4 with the 2000-step linear warm-up of the reference's launch scripts (src/train_cc12m_slurm.sh:28-29): a
    # constant 5e-4 from step 0 collapses the random-init model to uniform logits (loss = ln N) within ~20 steps
    sched = cosine_lr(opt, 5e-4, 2000, 200000)
    counter = {"n": 0}

    last_out = {}           # the model outputs of the last timed step, for --dump-outputs

    def step(keep_out=False):
        sched(counter["n"])
        counter["n"] += 1
        opt.zero_grad(set_to_none=True)
        out = model(images, texts)
        loss = loss_fn(**out, output_dict=True)["total_loss"]
        loss.backward()
        sync.sync()
        sync.wait()
        opt.step()
        ops.clamp1(model.logit_scale.data, 0.0, math.log(100))
        if keep_out:
            last_out.update(out)
        return loss

    def fence():
        if world > 1:
            torch.distributed.barrier()
        torch.cuda.synchronize()

    first_loss = None
    for _ in range(args.warmup):
        loss = step()
        if first_loss is None:
            first_loss = float(loss.detach())
    fence()
    t0 = time.perf_counter()
    for i in range(args.steps):
        loss = step(keep_out=bool(args.dump_outputs) and i == args.steps - 1)
    dt_host = time.perf_counter() - t0          # the host's share: every launch of the K steps is queued at this point
    fence()
    dt = time.perf_counter() - t0
    if world > 1:
        t = torch.tensor([dt], device=dev)
        torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.MAX)
        dt = float(t)
    final_loss = float(loss.detach())
    assert math.isfinite(final_loss), "training diverged"
    if first_loss is not None and args.warmup + args.steps >= 4:
        assert final_loss != first_loss, "the loss did not move: the optimizer step is not reaching the weights"
        assert abs(final_loss - math.log(args.global_batch)) > 1e-3 or abs(first_loss - math.log(args.global_batch)) < 1e-3, \
            "the model collapsed to uniform logits (loss = ln N)"
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, loss, last_out, model)
    last_out.clear()
    ms = dt / args.steps * 1e3
    ips = args.global_batch / (dt / args.steps)
    layout = model._text_engine.last_layout
    live_frac = (layout.rows / float(b * model.context_length)) if layout is not None else 1.0
    text_rows = f"packed {layout.rows_live}+{layout.rows - layout.rows_live} of {b * model.context_length}" if layout is not None else "dense"

    # ---- the same step with the reference's dense text layout (all 77 positions), a short second measurement
    dense = None
    if args.full and layout is not None and not args.no_dense_compare:
        model._text_engine.packed = False
        for _ in range(2):
            step()
        fence()
        t1 = time.perf_counter()
        nd = max(2, args.steps // 2)
        for _ in range(nd):
            step()
        fence()
        dd = (time.perf_counter() - t1) / nd
        if world > 1:
            t = torch.tensor([dd], device=dev)
            torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.MAX)
            dd = float(t)
        dense = {"ms_per_step": round(dd * 1e3, 3), "value": round(args.global_batch / dd, 1), "steps": nd}
        model._text_engine.packed = True
        step()

    if args.full:
        # ---- instrumented step: per-launch durations of the dominant kernel (bf16 NT GEMM).  The towers run on ONE
        # stream here: with the default two streams a launch's begin-to-end time includes CUs held by the other tower's
        # kernel, which says nothing about the kernel itself.
        prev_streams = os.environ.get("CLIPX_TOWER_STREAMS")
        os.environ["CLIPX_TOWER_STREAMS"] = "0"
        if prev_streams != "0":
            # activations now come from the main stream's allocator pool: release the side streams' cached blocks and
            # run one untimed step so that no hipMalloc sits between an event and its launch
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            step()
            torch.cuda.synchronize()
        timer = LaunchTimer()
        import colxlip_amd.model as M
        orig_f, orig_d = ops.linear_fwd, ops.linear_dgrad
        ops.linear_fwd = timer.wrap(orig_f, lambda x, w, *a, **k: 2.0 * x.shape[0] * x.shape[1] * w.shape[0], _fwd_bytes)
        ops.linear_dgrad = timer.wrap(orig_d, lambda dy, w, wt, *a, **k: 2.0 * dy.shape[0] * dy.shape[1] * (w.shape[1] if w is not None else wt.shape[0]), _dgrad_bytes)
        # precision fp8_mfma: the forward linears and dgrads of the residual blocks run on gemm_fp8_nt8p_kernel -- in that mode IT is
        # the dominant kernel, timed by itself and priced against the fp8 peak (the bf16 launches that remain -- patch embed,
        # projections, the pooled last block -- are reported beside it)
        timer8 = LaunchTimer()
        orig_f8, orig_d8 = ops.linear_fwd_fp8, ops.linear_dgrad_fp8
        ops.linear_fwd_fp8 = timer8.wrap(orig_f8, lambda x8, xe, w8, *a, **k: 2.0 * x8.shape[0] * x8.shape[1] * w8.shape[0], _fwd8_bytes)
        ops.linear_dgrad_fp8 = timer8.wrap(orig_d8, lambda d8, de, wt8, *a, **k: 2.0 * d8.shape[0] * d8.shape[1] * wt8.shape[0], _dgrad8_bytes)
        step()
        n_launch, gemm_ms, gemm_flops, gemm_bytes = timer.totals()
        n8, ms8, flops8, bytes8 = timer8.totals()
        ops.linear_fwd, ops.linear_dgrad = orig_f, orig_d
        ops.linear_fwd_fp8, ops.linear_dgrad_fp8 = orig_f8, orig_d8
        if prev_streams is None:
            del os.environ["CLIPX_TOWER_STREAMS"]
        else:
            os.environ["CLIPX_TOWER_STREAMS"] = prev_streams
        achieved = gemm_flops / (gemm_ms * 1e-3) / 1e12 if gemm_ms > 0 else 0.0

    if rank == 0:
        print(f"[bench] timed region done: {ms:.1f} ms/step", file=sys.stderr, flush=True)
        gf = FWD_BWD_GFLOP_PER_PAIR.get(args.model)
        headline = args.model == "ViT-B-32" and args.global_batch == 4096 and args.precision == "bf16"
        res = {
            # BASELINE.json's metric string only for BASELINE.json's workload; any other model / batch / precision says what it is
            "metric": "images/sec (whole node), ViT-B/32 global batch 4096 at 1/2/4/8 MI355X" if headline else
                      f"images/sec (whole node), {args.model} global batch {args.global_batch} {args.precision} on {world} MI355X "
                      "(not BASELINE.json's headline workload)",
            "value": round(ips, 1), "unit": "images/sec", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(ms, 3), "host_enqueue_ms_per_step": round(dt_host / args.steps * 1e3, 3),
            "higher_is_better": True, "scaling": "strong", "vs_baseline": None,
            "dtype": {"fp32": "f32", "fp8": "bf16 (fp8 e4m3 block weights)",
                      "fp8_mfma": "fp8 e4m3 forward GEMMs (fp8 MFMA), bf16 backward"}.get(args.precision, "bf16"), "data": "synthetic",
            "config": {"workload": f"{args.model} + 77-token text tower, {image_size if isinstance(image_size, int) else image_size[0]}px, global batch {args.global_batch} "
                                   f"(per-GPU {b}), full train step incl. AdamW, random init",
                       "global_batch": args.global_batch, "parallelism": f"dp{world}",
                       **({"rehearsal": f"{world} ranks sharing ONE GPU over gloo: code-path check, timings meaningless"}
                          if args.rehearse_on_one_gpu else {}),
                       "loss": ("ColClipLoss alpha 0.5 (global + MaxSim token contrastive), " + ("global logits on every rank + gather_with_grad" if (world > 1 and args.colclip_global) else ("each rank its text rows (rows_local) + gather_with_grad" if world > 1 else "single rank")))
                               if colxlip else ("local_loss+gather_with_grad" if world > 1 else "single-rank"),
                       **({"optimizer": "sharded (ZeRO-1)"} if shard else {}),
                       "grad_checkpointing": bool(args.grad_checkpointing),
                       "tower_streams": 1 if os.environ.get("CLIPX_TOWER_STREAMS", "1") == "0" else 2,
                       "text_rows": text_rows, "lr": "5e-4, 2000-step warm-up"},
            "first_loss": round(first_loss, 4) if first_loss is not None else None, "final_loss": round(final_loss, 4),
        }
        if args.full:
            res["roofline"] = {"bound": "mfma", "kernel": "NT GEMM (gemm_bf16_nt8p_kernel; gemm_bf16_nt_kernel / nt5 for the shapes it does not take)", "achieved": round(achieved, 1),
                               "peak": PEAK_BF16_DENSE_TFLOPS, "unit": "TFLOP/s", "frac": round(achieved / PEAK_BF16_DENSE_TFLOPS, 4),
                               "traffic": pmc_traffic(args.model, b, args.precision, "packed" if layout is not None else "dense"),
                               "algorithmic_bytes_per_launch": int(gemm_bytes / max(n_launch, 1)),
                               "launches_per_step": n_launch, "avg_launch_us": round(gemm_ms * 1e3 / max(n_launch, 1), 1)}
            if n8 > 0 and flops8 > gemm_flops:
                ach8 = flops8 / (ms8 * 1e-3) / 1e12
                res["roofline_bf16_launches"] = {k: res["roofline"][k] for k in ("kernel", "achieved", "peak", "frac", "launches_per_step", "avg_launch_us")}
                res["roofline"] = {"bound": "mfma", "kernel": "gemm_fp8_nt8p_kernel (e4m3 x e4m3 on v_mfma_f32_16x16x128_f8f6f4: forward linears + dgrads of the residual blocks)",
                                   "achieved": round(ach8, 1), "peak": PEAK_FP8_DENSE_TFLOPS, "unit": "TFLOP/s",
                                   "frac": round(ach8 / PEAK_FP8_DENSE_TFLOPS, 4), "traffic": None,
                                   "algorithmic_bytes_per_launch": int(bytes8 / n8), "launches_per_step": n8,
                                   "avg_launch_us": round(ms8 * 1e3 / n8, 1)}
            if res["roofline"]["traffic"]:
                res["roofline"]["traffic_over_algorithmic"] = round(res["roofline"]["traffic"] / max(1, res["roofline"]["algorithmic_bytes_per_launch"]), 3)
        if dense is not None:
            # positions behind a caption's EOT cannot reach the loss (causal mask + EOT pooling) and get a zero gradient:
            # `value` computes only the live positions; this is the same step computing all 77 like the reference does
            res["dense_text_rows"] = dense
        if gf:
            step_tf = ips * gf * 1e9 / 1e12 / world
            # BASELINE.md counts all 77 text positions; with packed rows the text tower executes live_frac of them
            txt_share = {"ViT-B-32": 5.96 / 14.78, "ViT-B-16": 5.96 / 41.09, "ViT-L-14-336": 13.30 / 395.2, "ViT-H-14": 47.09 / 381.7}[args.model]
            executed = gf * (1.0 - txt_share * (1.0 - live_frac))
            res["step_roofline"] = {"achieved_tflops_per_gpu": round(ips * executed * 1e9 / 1e12 / world, 1),
                                    "peak": PEAK_BF16_DENSE_TFLOPS,
                                    "frac": round(ips * executed * 1e9 / 1e12 / world / PEAK_BF16_DENSE_TFLOPS, 4),
                                    "flops_per_pair_executed": round(executed * 1e9), "flops_per_pair_dense_reference": gf * 1e9,
                                    "dense_equivalent_tflops_per_gpu": round(step_tf, 1)}
        if args.full and world == 1 and not args.no_cpu_baseline:
            res["cpu_baseline"] = cpu_baseline(args.cpu_steps)
        print(json.dumps(res), flush=True)
    if world > 1 or args.force_dist:
        torch.distributed.barrier()
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
