"""The RCCL ("nccl" backend) code path on the one GPU a test box has: a world-size-1 process group still runs every
collective the data-parallel step issues (all_gather_into_tensor / reduce_scatter_tensor in gather_features,
bucketed all_reduce on the side stream in GradSync, the early per-tower hook), so API misuse, stream fencing and
dtype/contiguity mistakes show up here rather than on the 8-GPU node.  Multi-rank semantics are covered on CPU with
gloo (tests/test_distributed_cpu.py)."""
import math
import os
import socket

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.fixture(scope="module")
def nccl_world1():
    import torch.distributed as dist
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    created = False
    if not dist.is_initialized():
        s = socket.socket()
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
        s.close()
        os.environ["MASTER_ADDR"] = "127.0.0.1"
        os.environ["MASTER_PORT"] = str(port)
        torch.cuda.set_device(0)
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
        created = True
    yield dist
    if created:
        dist.destroy_process_group()


def test_gather_features_rccl_single_rank(nccl_world1):
    from colxlip_amd.loss import ClipLoss, gather_features
    torch.manual_seed(0)
    img = torch.nn.functional.normalize(torch.randn(64, 32, device=DEV), dim=-1).requires_grad_(True)
    txt = torch.nn.functional.normalize(torch.randn(64, 32, device=DEV), dim=-1).requires_grad_(True)
    scale = torch.tensor(10.0, device=DEV, requires_grad=True)
    for local_loss in (False, True):
        for gwg in (False, True):
            ai, at = gather_features(img, txt, local_loss=local_loss, gather_with_grad=gwg, rank=0, world_size=1)
            assert torch.equal(ai, img) and torch.equal(at, txt)
    # gather_with_grad backward = reduce_scatter_tensor: identity on one rank
    ai, at = gather_features(img, txt, local_loss=True, gather_with_grad=True, rank=0, world_size=1)
    (ai.sum() * 2 + at.sum() * 3).backward()
    assert torch.allclose(img.grad, torch.full_like(img, 2.0)) and torch.allclose(txt.grad, torch.full_like(txt, 3.0))
    # the loss object on top of it agrees with the single-process loss
    img.grad = txt.grad = None
    ref = ClipLoss()(img, txt, scale)
    got = ClipLoss(local_loss=True, gather_with_grad=True, rank=0, world_size=1)(img, txt, scale)
    assert abs(float(ref) - float(got)) < 1e-6


def test_train_step_with_gradsync_on_rccl(nccl_world1):
    """Two full data-parallel train steps (early per-tower all-reduce hook + leftover buckets on the side stream + fused
    AdamW) through RCCL on one rank give the same losses as the same steps without the synchroniser."""
    from colxlip_amd import create_model_and_transforms, ops
    from colxlip_amd.data import synthetic_batch
    from colxlip_amd.distributed import GradSync
    from colxlip_amd.loss import ClipLoss
    from colxlip_amd.optim import FusedAdamW, param_groups

    def run(with_sync):
        torch.manual_seed(0)
        model, _, _ = create_model_and_transforms("ViT-small-test", precision="bf16", device=DEV, output_dict=True)
        model.train()
        opt = FusedAdamW(param_groups(model.named_parameters(), 0.2), lr=5e-4, betas=(0.9, 0.98), eps=1e-6)
        loss_fn = ClipLoss(local_loss=True, gather_with_grad=True, cache_labels=True, rank=0, world_size=1)
        sync = GradSync(list(model.parameters()), 1, bucket_mb=0.25, force=with_sync).attach(model)
        images, texts = synthetic_batch(16, model.visual.image_size, model.context_length, model.vocab_size, seed=7,
                                        device=DEV, image_dtype=torch.bfloat16)
        texts = texts[:, 0].contiguous()
        losses = []
        for _ in range(2):
            opt.zero_grad(set_to_none=True)
            out = model(images, texts)
            loss = loss_fn(**out, output_dict=True)["total_loss"]
            loss.backward()
            sync.sync()
            sync.wait()
            opt.step()
            ops.clamp1(model.logit_scale.data, 0.0, math.log(100))
            losses.append(float(loss))
        torch.cuda.synchronize()
        return losses

    a, b = run(False), run(True)
    assert all(math.isfinite(v) for v in b)
    # same arithmetic with and without the synchroniser
    assert all(abs(x - y) <= 1e-4 * max(1.0, abs(x)) for x, y in zip(a, b)), (a, b)


def test_sharded_optimizer_on_rccl_single_rank(nccl_world1, tmp_path):
    """`--shard-optimizer` (GradSync(shard_optimizer=True) + ShardedAdamW) through RCCL on one rank: the in-place
    reduce_scatter_tensor / all_gather_into_tensor calls, the flat parameter and moment arenas, the clipped variant and the
    checkpoint round trip -- weights after three steps equal the unsharded optimizer's, the state dict has the reference
    optimizer's keys with full-size moments, and a run resumed from it continues identically."""
    from colxlip_amd import create_model_and_transforms, ops
    from colxlip_amd.data import synthetic_batch
    from colxlip_amd.distributed import GradSync
    from colxlip_amd.loss import ClipLoss
    from colxlip_amd.optim import FusedAdamW, ShardedAdamW, clip_grad_norm_, param_groups, sharded_clip_grad_norm_

    def build(shard, wire=None):
        torch.manual_seed(0)
        model, _, _ = create_model_and_transforms("ViT-small-test", precision="fp32", device=DEV, output_dict=True)
        model.train()
        sync = GradSync(list(model.parameters()), 1, force=True, shard_optimizer=shard, grad_dtype=wire).attach(model)
        groups = param_groups(model.named_parameters(), 0.2)
        kw = dict(lr=1e-3, betas=(0.9, 0.98), eps=1e-6)
        opt = ShardedAdamW(groups, sync, **kw) if shard else FusedAdamW(groups, **kw)
        return model, sync, opt

    images, texts = synthetic_batch(16, 64, 77, 1024, seed=7, device=DEV, image_dtype=torch.float32)
    texts = texts[:, 0].contiguous()
    loss_fn = ClipLoss(local_loss=True, gather_with_grad=True, cache_labels=True, rank=0, world_size=1)

    def steps(model, sync, opt, n, clip, accumulate=False):
        for _ in range(n):
            opt.zero_grad(set_to_none=True)
            if accumulate:                       # a first micro-batch whose gradients stay local (train.py's no_sync scheme)
                with sync.no_sync():
                    loss_fn(**model(images.flip(0), texts), output_dict=True)["total_loss"].backward()
            loss = loss_fn(**model(images, texts), output_dict=True)["total_loss"]
            loss.backward()
            sync.sync()
            sync.wait()
            params = [p for p in model.parameters() if p.grad is not None]
            if clip is not None:
                (sharded_clip_grad_norm_(sync, params, clip) if sync.shard else clip_grad_norm_(params, clip))
            opt.step()
            ops.clamp1(model.logit_scale.data, 0.0, math.log(100))
        torch.cuda.synchronize()

    for clip in (None, 0.5):
        plain, sharded = build(False), build(True)
        eng = sharded[0].visual._engine
        assert eng.P["proj"].data_ptr() >= eng._param_arena.data_ptr()            # parameters now live in the flat arena
        steps(*plain, 3, clip)
        steps(*sharded, 3, clip)
        sd_a, sd_b = plain[0].state_dict(), sharded[0].state_dict()
        worst = max(float((sd_a[k] - sd_b[k]).abs().max()) for k in sd_a)
        # Same update -- up to what the unsharded optimizer differs from ITSELF run to run: the embedding backward adds with fp32
        # atomics, and AdamW's first steps turn an absolute difference of 1e-8 in a gradient of 1e-7 into lr * 1e-2 (the update is
        # g / (|g| + eps)).  Measured here instead of assumed.
        again = build(False)
        steps(*again, 3, clip)
        sd_c = again[0].state_dict()
        noise = max(float((sd_a[k] - sd_c[k]).abs().max()) for k in sd_a)
        assert worst < max(2e-5, 3.0 * noise), (clip, worst, noise)
    # gradient accumulation: the last backward reduce-scatters the accumulated arenas
    plain, sharded = build(False), build(True)
    steps(*plain, 2, 0.5, accumulate=True)
    steps(*sharded, 2, 0.5, accumulate=True)
    sd_a, sd_b = plain[0].state_dict(), sharded[0].state_dict()
    assert max(float((sd_a[k] - sd_b[k]).abs().max()) for k in sd_a) < 2e-5
    # bf16 on the wire (`--grad-comm-dtype bf16` with `--shard-optimizer`): gradients rounded once to bf16 -> the first AdamW step
    # (a sign-like update at step 1) moves every weight by at most ~lr either way; after one step the weights agree to a few lr/100
    a, b = build(True), build(True, torch.bfloat16)
    steps(*a, 1, None)
    steps(*b, 1, None)
    sd_a, sd_b = a[0].state_dict(), b[0].state_dict()
    mean = float(sum((sd_a[k] - sd_b[k]).abs().sum() for k in sd_a) / sum(v.numel() for v in sd_a.values()))
    assert mean < 2e-5, mean
    # checkpoint round trip of the sharded optimizer
    model, sync, opt = sharded
    opt.gather_state()
    osd = opt.state_dict()
    assert set(osd) == {"state", "param_groups"}
    some = osd["state"][0]
    assert set(some) == {"step", "exp_avg", "exp_avg_sq"} and some["step"] == 2          # the accumulation run above: two steps
    path = os.path.join(tmp_path, "opt.pt")
    torch.save({"model": model.state_dict(), "opt": osd}, path)
    steps(model, sync, opt, 1, 0.5)
    want = {k: v.clone() for k, v in model.state_dict().items()}
    model2, sync2, opt2 = build(True)
    ck = torch.load(path, map_location=DEV, weights_only=True)
    model2.load_state_dict(ck["model"])
    opt2.load_state_dict(ck["opt"])
    steps(model2, sync2, opt2, 1, 0.5)
    got = model2.state_dict()
    worst = max(float((want[k] - got[k]).abs().max()) for k in want)
    assert worst < 2e-5, worst


def test_early_gradient_ranges_are_complete_and_cover_the_arena():
    """The engines hand finished tails of their flat gradient arenas to the synchroniser while the backward is still
    running.  A stand-in hook doubles each range as it is handed over (what a 2-rank sum of identical gradients would
    do): if every range is complete at that point and the ranges tile each arena exactly once, every gradient ends up
    exactly twice the plain one; a kernel writing into a range after its hand-over would leave 1x there."""
    from colxlip_amd import create_model_and_transforms
    from colxlip_amd.data import synthetic_batch
    from colxlip_amd.loss import ClipLoss

    def grads(hooked):
        torch.manual_seed(0)
        model, _, _ = create_model_and_transforms("ViT-small-test", precision="bf16", device=DEV, output_dict=True)
        model.train()
        seen = []
        if hooked:
            def hook(view):
                seen.append((view.data_ptr(), view.numel()))
                view.mul_(2.0)                        # on the backward's own stream: ordered after the producing kernels
            for eng in (model.visual._engine, model._text_engine):
                eng.grad_ready_hook = hook
        images, texts = synthetic_batch(16, model.visual.image_size, model.context_length, model.vocab_size, seed=7,
                                        device=DEV, image_dtype=torch.bfloat16)
        out = model(images, texts[:, 0].contiguous())
        ClipLoss()(**out, output_dict=True)["total_loss"].backward()
        torch.cuda.synchronize()
        arenas = [(e._arena.data_ptr(), e._arena.numel()) for e in (model.visual._engine, model._text_engine)]
        g = {n: (p.grad.detach().clone(), any(b <= p.grad.data_ptr() < b + 4 * k for b, k in arenas))
             for n, p in model.named_parameters() if p.grad is not None}
        return g, seen, arenas

    plain, _, _ = grads(False)
    doubled, seen, arenas = grads(True)
    assert len(seen) >= 4, seen                         # several ranges per tower, not one per tower
    for base, numel in arenas:                          # the ranges of an arena are disjoint and tile it
        mine = sorted((p, n) for p, n in seen if base <= p < base + 4 * numel)
        assert mine and mine[0][0] == base
        end = base
        for p, n in mine:
            assert p == end, "gap or overlap between early ranges"
            end = p + 4 * n
        assert end == base + 4 * numel
    assert sum(inside for _, inside in doubled.values()) > 20
    for n, (g, _) in plain.items():
        got, inside = doubled[n]
        want = 2.0 * g if inside else g           # (atomics in some reductions: equal up to summation order)
        assert torch.allclose(got, want, rtol=1e-3, atol=1e-6 * float(want.abs().max() + 1e-30)), n


# ------------------------------------------------------------------ gradient accumulation x GradSync
def _small_model(precision="fp32"):
    from colxlip_amd import create_model_and_transforms
    torch.manual_seed(0)
    model, _, _ = create_model_and_transforms("ViT-small-test", precision=precision, device=DEV, output_dict=True)
    model.train()
    return model


def _two_batches(model, dtype=torch.float32):
    from colxlip_amd.data import synthetic_batch
    out = []
    for seed in (7, 8):
        im, tx = synthetic_batch(16, model.visual.image_size, model.context_length, model.vocab_size, seed=seed, device=DEV,
                                 image_dtype=dtype)
        out.append((im, tx[:, 0].contiguous()))
    return out


def _backward(model, batch):
    from colxlip_amd.loss import ClipLoss
    out = model(*batch)
    ClipLoss()(**out, output_dict=True)["total_loss"].backward()


def _plain_grads(batches):
    model = _small_model()
    res = []
    for b in batches:
        model.zero_grad(set_to_none=True)
        _backward(model, b)
        torch.cuda.synchronize()
        res.append({n: p.grad.detach().clone() for n, p in model.named_parameters()})
    return res


@pytest.mark.parametrize("mode", ["no_sync_then_reduce", "reduce_every_backward"])
def test_accumulation_with_gradsync_doubling_stand_in(nccl_world1, mode):
    """Two accumulated backwards through the real GradSync (side stream, fences, early ranges, sync() for what is outside
    the arenas) with the collective replaced by `x *= 2` -- what a mean over two ranks does when the other rank's local
    gradient is 3x ours.  train.py's scheme (first micro-batch inside no_sync()) must give 2*(g0+g1) everywhere; DDP's
    scheme (reduce in every backward) must give 4*g0 + 2*g1: each range reduced exactly once per backward, after that
    backward's accumulation into it and before the next one's.  Round 1 produced mean(g0) + local(g1) here."""
    from colxlip_amd.distributed import GradSync
    model = _small_model()
    batches = _two_batches(model)
    g0, g1 = _plain_grads(batches)
    sync = GradSync(list(model.parameters()), 1, bucket_mb=0.25, force=True).attach(model)
    sync._reduce_flat = lambda flat: flat.mul_(2.0)
    model.zero_grad(set_to_none=True)
    if mode == "no_sync_then_reduce":
        with sync.no_sync():
            _backward(model, batches[0])
        _backward(model, batches[1])
        want = {n: 2.0 * (g0[n] + g1[n]) for n in g0}
    else:
        _backward(model, batches[0])
        _backward(model, batches[1])
        want = {n: 4.0 * g0[n] + 2.0 * g1[n] for n in g0 if n != "logit_scale"}
        want["logit_scale"] = 2.0 * (g0["logit_scale"] + g1["logit_scale"])      # outside the arenas: only sync() sees it
    sync.sync()
    sync.wait()
    torch.cuda.synchronize()
    assert sync.stats["early_ranges"] >= 4
    for n, p in model.named_parameters():
        w = want[n]
        assert torch.allclose(p.grad, w, rtol=2e-4, atol=1e-6 * float(w.abs().max() + 1e-30)), (mode, n)


def test_ddp_wrapped_model_matches_plain(nccl_world1, monkeypatch):
    """reference main.py:264-271 wraps the factory's model in DistributedDataParallel.  Here DDP keeps logit_scale only; the
    towers' arenas are averaged by the engines' own hooks inside the backward (no sync()/wait() call anywhere).  On a
    one-rank RCCL group the result must equal the unwrapped model's gradients, for a plain step and for two accumulated
    backwards, and the hooks must really have run."""
    monkeypatch.setenv("CLIPX_FORCE_SYNC", "1")
    model = _small_model()
    batches = _two_batches(model)
    g0, g1 = _plain_grads(batches)
    ddp = torch.nn.parallel.DistributedDataParallel(model, device_ids=[torch.device("cuda", 0)])
    ignored = ddp.parameters_to_ignore
    assert "visual.conv1.weight" in ignored and "token_embedding.weight" in ignored and "logit_scale" not in ignored
    # what the REDUCER is built over (DDP matches f"{module_name}.{param_name}" there: ".positional_embedding" for a parameter
    # held directly by the wrapped module -- listing only "positional_embedding" left it, and text_projection, with the reducer,
    # which then copied a stale bucket over the gradient in the accumulating backward below)
    reducer_params, _ = ddp._build_params_for_reducer()
    assert len(reducer_params) == 1 and reducer_params[0] is model.logit_scale
    ddp.zero_grad(set_to_none=True)
    _backward(ddp, batches[0])
    torch.cuda.synchronize()
    gs = model._auto_sync
    assert gs is not None and gs.fence_in_backward and gs.stats["early_ranges"] >= 4
    for n, p in model.named_parameters():
        assert torch.allclose(p.grad, g0[n], rtol=2e-4, atol=1e-6 * float(g0[n].abs().max() + 1e-30)), n
    _backward(ddp, batches[1])                      # accumulate, as the reference's accum loop does under DDP
    torch.cuda.synchronize()
    for n, p in model.named_parameters():
        w = g0[n] + g1[n]
        assert torch.allclose(p.grad, w, rtol=2e-4, atol=1e-6 * float(w.abs().max() + 1e-30)), n


def test_bf16_gradient_buckets_on_the_wire(nccl_world1):
    """grad_dtype=bf16: pack -> all-reduce(AVG) -> unpack over the fp32 arena; one rank => every gradient equals its own
    bf16 rounding."""
    from colxlip_amd.distributed import GradSync
    model = _small_model()
    batches = _two_batches(model)
    (g0,) = _plain_grads(batches[:1])
    sync = GradSync(list(model.parameters()), 1, bucket_mb=0.25, force=True, grad_dtype=torch.bfloat16).attach(model)
    model.zero_grad(set_to_none=True)
    _backward(model, batches[0])
    sync.sync()
    sync.wait()
    torch.cuda.synchronize()
    checked = 0
    for n, p in model.named_parameters():
        if n == "logit_scale":
            continue
        want = g0[n].to(torch.bfloat16).float()
        assert torch.allclose(p.grad, want, rtol=1e-2, atol=1e-6 * float(want.abs().max() + 1e-30)), n
        checked += 1
    assert checked > 50


def test_tower_called_twice_in_one_graph():
    """two encode_image calls before ONE backward -- both autograd nodes run before any .grad is installed;
    the second must not overwrite the first one's gradient views in the shared arena.  Expected: g_A + g_B."""
    model = _small_model()
    batches = _two_batches(model)
    w = torch.randn(16, model.visual.output_dim, device=DEV, generator=torch.Generator(device=DEV).manual_seed(1))
    singles = []
    for im, _ in batches:
        model.zero_grad(set_to_none=True)
        (model.encode_image(im, normalize=True) * w).sum().backward()
        torch.cuda.synchronize()
        singles.append({n: p.grad.detach().clone() for n, p in model.visual.named_parameters()})
    assert float(singles[0]["conv1.weight"].abs().max()) > 0
    model.zero_grad(set_to_none=True)
    ((model.encode_image(batches[0][0], normalize=True) * w).sum()
     + (model.encode_image(batches[1][0], normalize=True) * w).sum()).backward()
    torch.cuda.synchronize()
    for n, p in model.visual.named_parameters():
        w = singles[0][n] + singles[1][n]
        assert torch.allclose(p.grad, w, rtol=2e-4, atol=1e-6 * float(w.abs().max() + 1e-30)), n
