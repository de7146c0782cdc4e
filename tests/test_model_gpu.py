"""Model-level parity on the GPU: the HIP towers + loss (through the drop-in API) against the CPU
oracle and the committed golden fixtures generated from the reference's own files.
Bar (BASELINE.json north_star): logits and loss within 1e-3 (fp32) on identical synthetic batches."""
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import colxlip_amd  # noqa: E402
from colxlip_amd import create_model_and_transforms  # noqa: E402
from colxlip_amd.loss import ClipLoss  # noqa: E402
from colxlip_amd.optim import FusedAdamW, param_groups  # noqa: E402
from oracle import clip_oracle as O  # noqa: E402

DEV = "cuda"


def _load(golden_dir, name):
    z = np.load(os.path.join(golden_dir, name), allow_pickle=False)
    return {k: z[k] for k in z.files}


def _t(a):
    return torch.from_numpy(np.asarray(a))


def build(model_name, sd, precision):
    model, _, _ = create_model_and_transforms(model_name, precision=precision, device=DEV, output_dict=True)
    missing = model.load_state_dict({k: v.clone() for k, v in sd.items()}, strict=True)
    assert not missing.missing_keys and not missing.unexpected_keys
    model.train()
    return model


def run_step(model, image, text):
    model.zero_grad(set_to_none=True)
    out = model(image.to(DEV), text.to(DEV))
    loss = ClipLoss()(**out, output_dict=True)["total_loss"]
    loss.backward()
    grads = {k: p.grad.detach().float().cpu() for k, p in model.named_parameters()}
    return {k: (v.detach().float().cpu() if torch.is_tensor(v) else v) for k, v in out.items()}, float(loss), grads


def test_state_dict_schema():
    model, _, _ = create_model_and_transforms("ViT-B-32", precision="fp32", device="cpu")
    sd = O.init_state_dict(O.VIT_B_32, seed=0)
    msd = model.state_dict()
    assert set(msd.keys()) == set(sd.keys())
    assert all(tuple(msd[k].shape) == tuple(sd[k].shape) for k in sd)
    assert sum(p.numel() for p in model.parameters()) == 151277313


def test_tiny_fp32_matches_reference_golden(golden_dir):
    z = _load(golden_dir, "tiny_clip.npz")
    sd = {k[3:]: _t(v) for k, v in z.items() if k.startswith("sd/")}
    model = build("ViT-tiny-test", sd, "fp32")
    out, loss, grads = run_step(model, _t(z["image"]), _t(z["text"]))
    assert float((out["image_features"] - _t(z["image_features"])).abs().max()) < 1e-5
    assert float((out["text_features"] - _t(z["text_features"])).abs().max()) < 1e-5
    assert abs(loss - float(z["loss"])) < 1e-5
    worst = 0.0
    for k in sd:
        ref = _t(z["grad/" + k])
        err = float((grads[k] - ref).abs().max()) / (float(ref.abs().max()) + 1e-8)
        worst = max(worst, err)
        assert err < 2e-3, (k, err)
    print("tiny fp32 worst relative grad error", worst)


def test_tiny_fp32_quickgelu(golden_dir):
    z = _load(golden_dir, "tiny_clip.npz")
    q = _load(golden_dir, "tiny_clip_quickgelu.npz")
    sd = {k[3:]: _t(v) for k, v in z.items() if k.startswith("sd/")}
    model, _, _ = create_model_and_transforms("ViT-tiny-test", precision="fp32", device=DEV, output_dict=True,
                                              force_quick_gelu=True)
    model.load_state_dict(sd)
    out, loss, grads = run_step(model, _t(z["image"]), _t(z["text"]))
    assert abs(loss - float(q["loss"])) < 1e-5
    for k in ("visual.conv1.weight", "token_embedding.weight", "logit_scale"):
        ref = _t(q["grad/" + k])
        assert float((grads[k] - ref).abs().max()) < 2e-3 * (float(ref.abs().max()) + 1e-8), k


def test_b32_fp32_logits_and_loss_within_1e3(golden_dir):
    """The north_star bar: ViT-B/32 at real size, logits/loss within 1e-3 of the reference CPU path."""
    z = _load(golden_dir, "b32_batch4.npz")
    cfg = O.VIT_B_32
    sd = O.perturb_state_dict(O.init_state_dict(cfg, seed=0), seed=1)
    chk = np.array([float(sd[k].double().sum()) for k in sorted(sd.keys())])
    assert np.allclose(chk, z["sd_checksum"], rtol=1e-9, atol=1e-9)
    image, text = O.synthetic_batch(cfg, 4, seed=1234)
    model = build("ViT-B-32", sd, "fp32")
    out, loss, grads = run_step(model, image, text)
    logits = float(out["logit_scale"]) * out["image_features"] @ out["text_features"].t()
    err_logits = float((logits - _t(z["logits"])).abs().max())
    print("B/32 fp32: max |logit err|", err_logits, "loss err", abs(loss - float(z["loss"])))
    assert err_logits < 1e-3
    assert abs(loss - float(z["loss"])) < 1e-3
    assert float((out["image_features"] - _t(z["image_features"])).abs().max()) < 1e-4
    assert float((out["text_features"] - _t(z["text_features"])).abs().max()) < 1e-4
    for name, norm in zip(z["grad_names"], z["grad_norms"]):
        g = grads[str(name)]
        assert abs(float(g.double().norm()) - norm) <= 5e-3 * norm + 1e-7, (name, float(g.double().norm()), norm)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_small_model_vs_oracle(precision):
    """width-128 / head-64 model (the MFMA attention path in bf16), batch 6, vs the CPU oracle."""
    cfg = O.ClipCfg(embed_dim=64, image_size=64, patch_size=16, vision_width=128, vision_layers=2,
                    context_length=77, vocab_size=1024, text_width=128, text_heads=2, text_layers=2)
    sd = O.perturb_state_dict(O.init_state_dict(cfg, seed=3), seed=4)
    image, text = O.synthetic_batch(cfg, 6, seed=99)
    ref_out, ref_loss, ref_grads = O.loss_and_grads(sd, image, text, cfg)
    model = build("ViT-small-test", sd, precision)
    out, loss, grads = run_step(model, image, text)
    ftol, ltol, gtol = (1e-5, 1e-5, 2e-3) if precision == "fp32" else (3e-2, 5e-2, 0.15)
    assert float((out["image_features"] - ref_out["image_features"]).abs().max()) < ftol
    assert float((out["text_features"] - ref_out["text_features"]).abs().max()) < ftol
    assert abs(loss - float(ref_loss)) < ltol
    for k in sd:
        ref = ref_grads[k]
        if float(ref.norm()) > 1e-4:
            rel = float((grads[k] - ref).norm() / (ref.norm() + 1e-8))
            assert rel < gtol, (k, rel)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("name,cfg", [
    ("ViT-hd80-test", dict(embed_dim=64, image_size=56, patch_size=14, vision_width=160, vision_layers=2,
                           vision_head_width=80, context_length=77, vocab_size=1024, text_width=160, text_heads=2,
                           text_layers=2)),
    ("ViT-long-test", dict(embed_dim=64, image_size=336, patch_size=14, vision_width=128, vision_layers=1,
                           context_length=77, vocab_size=1024, text_width=128, text_heads=2, text_layers=1)),
])
def test_other_family_shapes_vs_oracle(precision, name, cfg):
    """Scaled-down stand-ins for the shapes of the larger configs (ViT-H/14 has head dim 80, ViT-L/14-336 has
    577 image tokens, patch 14 -> K = 588 needs padding in bf16): full step vs the CPU oracle."""
    cfg = O.ClipCfg(**cfg)
    sd = O.perturb_state_dict(O.init_state_dict(cfg, seed=5), seed=6)
    image, text = O.synthetic_batch(cfg, 4, seed=11)
    ref_out, ref_loss, ref_grads = O.loss_and_grads(sd, image, text, cfg)
    model = build(name, sd, precision)
    out, loss, grads = run_step(model, image, text)
    ftol, ltol, gtol = (1e-5, 1e-5, 2e-3) if precision == "fp32" else (3e-2, 5e-2, 0.15)
    assert float((out["image_features"] - ref_out["image_features"]).abs().max()) < ftol
    assert float((out["text_features"] - ref_out["text_features"]).abs().max()) < ftol
    assert abs(loss - float(ref_loss)) < ltol
    for k in sd:
        ref = ref_grads[k]
        if float(ref.norm()) > 1e-4:
            rel = float((grads[k] - ref).norm() / (ref.norm() + 1e-8))
            assert rel < gtol, (k, rel)


def test_grad_accumulation_and_checkpointing(golden_dir):
    """second backward without zero_grad accumulates (beta=1 path); grad checkpointing is bit-identical."""
    z = _load(golden_dir, "tiny_clip.npz")
    sd = {k[3:]: _t(v) for k, v in z.items() if k.startswith("sd/")}
    model = build("ViT-tiny-test", sd, "fp32")
    image, text = _t(z["image"]).to(DEV), _t(z["text"]).to(DEV)
    _, _, g1 = run_step(model, image, text)
    out = model(image, text)
    ClipLoss()(**out).backward()          # no zero_grad: accumulates into existing .grad
    for k, p in model.named_parameters():
        assert torch.allclose(p.grad.cpu(), 2 * g1[k], rtol=1e-4, atol=1e-7), k
    model.set_grad_checkpointing(True)
    # every block recomputed (the reference's behaviour), one block kept whole, and the automatic split (everything fits here):
    # the same gradients whichever blocks are recomputed
    for keep in ("0", "1", ""):
        os.environ["CLIPX_CKPT_KEEP"] = keep
        try:
            _, _, g2 = run_step(model, image, text)
        finally:
            os.environ.pop("CLIPX_CKPT_KEEP", None)
        for k in g1:
            assert torch.allclose(g2[k], g1[k], rtol=1e-4, atol=1e-7), (keep, k)


def test_checkpoint_split_budget_and_oom_fallback(golden_dir, monkeypatch):
    """The automatic checkpoint split (`_Engine._ckpt_keep`, advisor finding round 3): (a) a deliberately small memory budget
    yields keep = 0 -- the reference's every-block recompute -- and the same gradients; (b) training state that does not exist
    yet (gradient arena, Adam moments, operand copies of BOTH towers) is taken off the budget before activations are kept;
    (c) an out-of-memory error while blocks are kept drops the split to 0 and the forward runs again: same gradients."""
    z = _load(golden_dir, "tiny_clip.npz")
    sd = {k[3:]: _t(v) for k, v in z.items() if k.startswith("sd/")}
    image, text = _t(z["image"]).to(DEV), _t(z["text"]).to(DEV)
    model = build("ViT-tiny-test", sd, "fp32")
    _, _, g_ref = run_step(model, image, text)
    eng_v, eng_t = model.visual._engine, model._text_engine
    assert eng_v.peer is eng_t and eng_t.peer is eng_v
    assert eng_v._state_bytes_to_come() == 0                       # a backward has run: arena (and moments) are accounted for
    fresh = build("ViT-tiny-test", sd, "bf16")
    n_v = sum(p.numel() for p in fresh.visual.parameters())
    assert fresh.visual._engine._state_bytes_to_come() == 16 * n_v   # 4 B gradients + 8 B moments + 2 x 2 B operand copies
    model.set_grad_checkpointing(True)
    real = torch.cuda.mem_get_info

    def small(dev=None):                                            # ~nothing free: every block must be recomputed
        free, total = real(dev)
        return (torch.cuda.memory_allocated() - torch.cuda.memory_reserved() + (1 << 16), total)
    monkeypatch.setattr(torch.cuda, "mem_get_info", small)
    for e in (eng_v, eng_t):
        e._keep_cache = None
    _, _, g_small = run_step(model, image, text)
    assert eng_v._keep_cache[1] == 0 and eng_t._keep_cache[1] == 0
    monkeypatch.setattr(torch.cuda, "mem_get_info", real)
    for e in (eng_v, eng_t):
        e._keep_cache = None
    # (c) the first kept block's forward "runs out of memory" once
    calls = {"n": 0}
    orig = type(eng_v)._block_fwd

    def flaky(self, *a, **k):
        if self is eng_v and calls["n"] == 0:
            calls["n"] += 1
            raise torch.cuda.OutOfMemoryError("injected")
        return orig(self, *a, **k)
    monkeypatch.setattr(type(eng_v), "_block_fwd", flaky)
    _, _, g_oom = run_step(model, image, text)
    assert calls["n"] == 1 and eng_v._keep_cache[1] == 0 and eng_t._keep_cache[1] == eng_t.layers
    for k in g_ref:
        assert torch.allclose(g_small[k], g_ref[k], rtol=1e-4, atol=1e-7), k
        assert torch.allclose(g_oom[k], g_ref[k], rtol=1e-4, atol=1e-7), k


def test_no_grad_forward_keeps_no_activations():
    """Evaluation / the accumulation path's feature-caching pass run under torch.no_grad(): inside Function.forward
    `ctx.needs_input_grad` is still True for parameters there, so the grad mode is read at the call site -- a no_grad forward
    must not hold the blocks' activations (nor write pre-activations): same features, a fraction of the training forward's memory."""
    from colxlip_amd import create_model_and_transforms
    from colxlip_amd.data import synthetic_batch
    torch.manual_seed(0)
    model, _, _ = create_model_and_transforms("ViT-B-32", precision="bf16", device=DEV, output_dict=True)      # 12 blocks per tower
    model.train()
    image, text = synthetic_batch(128, 224, 77, 49408, seed=9, device=DEV, image_dtype=torch.bfloat16)
    text = text[:, 0].contiguous()
    model(image, text)                                           # warm the allocator and the weight copies
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out_train = model(image, text)
    held_train = torch.cuda.memory_allocated() - base            # activations kept for the backward
    del out_train
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    with torch.no_grad():
        out_eval = model(image, text)
    peak_eval = torch.cuda.max_memory_allocated() - base
    assert model.visual._engine._grad_mode is False
    assert held_train > 200 * 2**20 and peak_eval < 0.3 * held_train, (held_train, peak_eval)      # ~one block's working set against twelve blocks' activations
    out_again = model(image, text)
    assert torch.equal(out_eval["image_features"], out_again["image_features"].detach())
    assert torch.equal(out_eval["text_features"], out_again["text_features"].detach())


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_packed_text_rows_equal_dense_layout(precision):
    """The text tower computes only positions 0..EOT of each caption (packed rows); CLIPX_TEXT_UNPAD=0 / engine.packed =
    False keeps the reference's dense [batch, 77] layout.  Same features and same gradients either way (positions behind
    the EOT are dead under the causal mask + EOT pooling): fp32 to summation order, bf16 to rounding."""
    cfg = O.ClipCfg(embed_dim=64, image_size=64, patch_size=16, vision_width=128, vision_layers=2,
                    context_length=77, vocab_size=1024, text_width=128, text_heads=2, text_layers=2)
    sd = O.perturb_state_dict(O.init_state_dict(cfg, seed=3), seed=4)
    image, text = O.synthetic_batch(cfg, 24, seed=5)
    res = {}
    for packed in (True, False):
        model = build("ViT-small-test", sd, precision)
        model._text_engine.packed = packed
        out, loss, grads = run_step(model, image, text)
        assert (model._text_engine.last_layout is not None) == packed
        res[packed] = (out, loss, grads)
    (o1, l1, g1), (o0, l0, g0) = res[True], res[False]
    ftol, gtol = (2e-6, 2e-4) if precision == "fp32" else (2e-3, 3e-2)
    assert float((o1["text_features"] - o0["text_features"]).abs().max()) < ftol
    assert abs(l1 - l0) < (1e-6 if precision == "fp32" else 2e-3)
    for k in g0:
        if float(g0[k].norm()) > 1e-6:
            rel = float((g1[k] - g0[k]).norm() / g0[k].norm())
            assert rel < gtol, (k, rel)


def test_packed_layout_follows_every_new_batch():
    """The packed-row layout is cached for a REPLAYED tensor object only.  Fresh batches -- even ones that land on the
    device address of the batch before (the caching allocator recycles it) -- get their own layout; an in-place edit of a
    replayed tensor (version bump) as well."""
    cfg = O.ClipCfg(embed_dim=64, image_size=64, patch_size=16, vision_width=128, vision_layers=2,
                    context_length=77, vocab_size=1024, text_width=128, text_heads=2, text_layers=2)
    sd = O.perturb_state_dict(O.init_state_dict(cfg, seed=3), seed=4)
    model = build("ViT-small-test", sd, "fp32")
    dense = build("ViT-small-test", sd, "fp32")
    dense._text_engine.packed = False
    ptrs = set()
    with torch.no_grad():
        for seed in (1, 2, 3):
            _, text = O.synthetic_batch(cfg, 16, seed=seed)
            t = text.to(DEV)
            ptrs.add(t.data_ptr())
            got = model.encode_text(t, normalize=True)
            want = dense.encode_text(t, normalize=True)
            assert float((got - want).abs().max()) < 2e-6, seed
            first = model._text_engine.last_layout
            assert model.encode_text(t, normalize=True) is not None and model._text_engine.last_layout is first   # replay: reused
            t[0] = torch.roll(t[0], 5)                       # in-place edit: EOT of caption 0 moves
            got = model.encode_text(t, normalize=True)
            assert model._text_engine.last_layout is not first
            assert float((got - dense.encode_text(t, normalize=True)).abs().max()) < 2e-6
            del t, got, want
    print("distinct device addresses over 3 batches:", len(ptrs))


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("ckpt", [False, True])
def test_last_block_on_pooled_rows_equals_dense(precision, ckpt, monkeypatch):
    """Only the CLS / EOT row of the last residual block's output is consumed (transformer.py:695,851): by default its
    out_proj, MLP and their backward run on `batch` rows.  engine.prune_last = False computes every token: same features,
    same gradients (also with per-block recompute)."""
    cfg = O.ClipCfg(embed_dim=64, image_size=64, patch_size=16, vision_width=128, vision_layers=2,
                    context_length=77, vocab_size=1024, text_width=128, text_heads=2, text_layers=2)
    sd = O.perturb_state_dict(O.init_state_dict(cfg, seed=3), seed=4)
    image, text = O.synthetic_batch(cfg, 12, seed=8)
    res = {}
    monkeypatch.setenv("CLIPX_CKPT_KEEP", "0")           # with ckpt: recompute every block (at this size all of them would fit)
    for prune in (True, "one in_proj GEMM", False):
        model = build("ViT-small-test", sd, precision)
        model.set_grad_checkpointing(ckpt)
        model.visual._engine.prune_last = bool(prune)
        model._text_engine.prune_last = bool(prune)
        if prune == "one in_proj GEMM":                      # the pooled block with q | k | v in one GEMM (the form fp8 modes use)
            model.visual._engine.pooled_split = False
            model._text_engine.pooled_split = False
        res[prune] = run_step(model, image, text)
    for variant in (True, "one in_proj GEMM"):
        _compare_pruned(res[variant], res[False], precision)


def _compare_pruned(r1, r0, precision):
    (o1, l1, g1), (o0, l0, g0) = r1, r0
    # bf16: the pooled block's attention is a different kernel (one query row, fp32 probabilities) from the dense block's (MFMA,
    # bf16 probabilities); each is 2-3e-3 from the fp32 run on this model (features) and they differ from each other by as much
    ftol, gtol = (2e-6, 2e-4) if precision == "fp32" else (4e-3, 3e-2)
    for k in ("image_features", "text_features"):
        assert float((o1[k] - o0[k]).abs().max()) < ftol, k
    assert abs(l1 - l0) < (1e-6 if precision == "fp32" else 4e-3)          # (bf16: 1.4e-3 and 0.9e-3 from the fp32 loss, opposite signs)
    for k in g0:
        if float(g0[k].norm()) > 1e-6:
            rel = float((g1[k] - g0[k]).norm() / g0[k].norm())
            assert rel < gtol, (k, rel)


def _fake_quant_e4m3(w):
    """per output channel: e = ceil(log2(amax / 448)), value = e4m3(w * 2^-e) * 2^e (round to nearest even, no saturation)"""
    w2 = w.reshape(w.shape[0], -1).double()
    amax = w.reshape(w.shape[0], -1).abs().amax(dim=1)
    fr, ex = torch.frexp(amax)                       # amax = fr * 2^ex, fr in [0.5, 1); 448 = 0.875 * 2^9
    e = torch.where(amax > 0, torch.where(fr <= 0.875, ex - 9, ex - 8), torch.zeros_like(ex)).to(torch.int32)
    scaled = (w2 * torch.pow(2.0, -e.double()).unsqueeze(1)).float()
    q = scaled.to(torch.float8_e4m3fn)
    return (q.float().double() * torch.pow(2.0, e.double()).unsqueeze(1)).float().reshape(w.shape), q, e


def test_fp8_weight_precision():
    """BASELINE config 5's operand format on the width-128 model: precision 'fp8' = e4m3 attention / MLP weights with a
    power-of-two scale per output channel, bf16 activations.  (a) the exported fp8 bytes + exponents equal torch's own
    float8_e4m3fn rounding of the same scaled weights, bit for bit; (b) the step equals the bf16 model loaded with the
    dequantised weights (same kernels, same operand values: the dequantised values are exact in bf16); (c) against the fp32
    CPU oracle run on the dequantised weights, bf16 tolerances (features 3e-2, loss 5e-2, gradients 15 % of norm)."""
    cfg = O.ClipCfg(embed_dim=64, image_size=64, patch_size=16, vision_width=128, vision_layers=2,
                    context_length=77, vocab_size=1024, text_width=128, text_heads=2, text_layers=2)
    sd = O.perturb_state_dict(O.init_state_dict(cfg, seed=3), seed=4)
    image, text = O.synthetic_batch(cfg, 8, seed=31)
    m8 = build("ViT-small-test", sd, "fp8")
    out8, loss8, g8 = run_step(m8, image, text)
    exported = m8.export_fp8_weights()
    suffixes = ("attn.in_proj_weight", "attn.out_proj.weight", "mlp.c_fc.weight", "mlp.c_proj.weight")
    sd_q = {}
    for k, v in sd.items():
        if k.endswith(suffixes):
            deq, q, e = _fake_quant_e4m3(v)
            sd_q[k] = deq
            w8, rexp = exported[k]
            assert torch.equal(w8.cpu().view(torch.float8_e4m3fn).float(), q.float()), k
            assert torch.equal(rexp.cpu(), e), k
            assert torch.equal(deq.to(torch.bfloat16).float(), deq), "dequantised e4m3 x 2^e must be exact in bf16"
        else:
            sd_q[k] = v
    assert len(exported) == 4 * (cfg.vision_layers + cfg.text_layers)
    m16 = build("ViT-small-test", sd_q, "bf16")
    # "same kernels": the quantised model runs its last block's in_proj as one GEMM (a quantised weight is not split into q and
    # k | v rows), so the bf16 twin does too
    m16.visual._engine.pooled_split = False
    m16._text_engine.pooled_split = False
    out16, loss16, g16 = run_step(m16, image, text)
    assert float((out8["image_features"] - out16["image_features"]).abs().max()) < 1e-6
    assert float((out8["text_features"] - out16["text_features"]).abs().max()) < 1e-6
    assert abs(loss8 - loss16) < 1e-6
    for k in g16:
        if float(g16[k].norm()) > 1e-6:
            assert float((g8[k] - g16[k]).norm() / g16[k].norm()) < 1e-3, k     # atomics in the embedding backward only
    ref_out, ref_loss, ref_grads = O.loss_and_grads(sd_q, image, text, cfg)
    assert float((out8["image_features"] - ref_out["image_features"]).abs().max()) < 3e-2
    assert abs(loss8 - float(ref_loss)) < 5e-2
    for k in sd:
        if float(ref_grads[k].norm()) > 1e-4:
            assert float((g8[k] - ref_grads[k]).norm() / ref_grads[k].norm()) < 0.15, k


def test_loss_matches_golden(golden_dir):
    z = _load(golden_dir, "loss_w1.npz")
    for tag in ("a", "b"):
        fi = _t(z[f"{tag}/image_features"]).to(DEV).requires_grad_(True)
        ft = _t(z[f"{tag}/text_features"]).to(DEV).requires_grad_(True)
        ls = _t(z[f"{tag}/log_logit_scale"]).to(DEV).requires_grad_(True)
        mod = ClipLoss()
        loss = mod(fi, ft, ls.exp())
        loss.backward()
        assert abs(float(loss) - float(z[f"{tag}/loss"])) < 1e-5
        assert float((fi.grad.cpu() - _t(z[f"{tag}/grad_image"])).abs().max()) < 1e-6
        assert float((ft.grad.cpu() - _t(z[f"{tag}/grad_text"])).abs().max()) < 1e-6
        assert abs(float(ls.grad) - float(z[f"{tag}/grad_log_logit_scale"])) < 1e-4
        li, lt = mod.get_logits(fi.detach(), ft.detach(), ls.detach().exp())
        assert float((li.cpu() - _t(z[f"{tag}/logits_per_image"])).abs().max()) < 1e-4
        assert float((lt.cpu() - _t(z[f"{tag}/logits_per_text"])).abs().max()) < 1e-4


def test_three_train_steps_match_oracle(golden_dir):
    """zero_grad -> fwd -> loss -> bwd -> fused AdamW -> clamp, three steps, fp32, vs the oracle."""
    z = _load(golden_dir, "tiny_clip.npz")
    sd = {k[3:]: _t(v) for k, v in z.items() if k.startswith("sd/")}
    batches = [O.synthetic_batch(O.TINY, 8, seed=s) for s in (1, 2, 3)]
    ref_params, ref_losses = O.train_steps(sd, batches, O.TINY, lr=5e-4, beta1=0.9, beta2=0.98, eps=1e-6, wd=0.2)
    model = build("ViT-tiny-test", sd, "fp32")
    opt = FusedAdamW(param_groups(model.named_parameters(), 0.2), lr=5e-4, betas=(0.9, 0.98), eps=1e-6)
    loss_fn = ClipLoss()
    losses = []
    for image, text in batches:
        opt.zero_grad()
        out = model(image.to(DEV), text.to(DEV))
        loss = loss_fn(**out)
        loss.backward()
        opt.step()
        with torch.no_grad():
            colxlip_amd.ops.clamp1(model.logit_scale, 0.0, math.log(100))
        losses.append(float(loss))
    assert np.allclose(losses, ref_losses, atol=2e-4), (losses, ref_losses)
    for k, p in model.named_parameters():
        assert float((p.detach().cpu() - ref_params[k]).abs().max()) < 5e-4, k


def test_bf16_weight_copies_follow_the_optimizer():
    """The fused AdamW writes parameters through raw pointers; the engines' bf16 copies of the weights (and their
    transposes) are keyed on Tensor._version, so the optimizer must bump it -- otherwise every step after the first
    runs on the initial weights.  After step + forward each copy must equal the CURRENT parameter rounded to bf16."""
    torch.manual_seed(0)
    model, _, _ = create_model_and_transforms("ViT-small-test", precision="bf16", device=DEV, output_dict=True)
    model.train()
    opt = FusedAdamW(param_groups(model.named_parameters(), 0.2), lr=1e-2, betas=(0.9, 0.98), eps=1e-6)
    from colxlip_amd.data import synthetic_batch
    images, texts = synthetic_batch(8, model.visual.image_size, model.context_length, model.vocab_size, seed=3, device=DEV,
                                    image_dtype=torch.bfloat16)
    texts = texts[:, 0].contiguous()
    losses = []
    for _ in range(3):
        opt.zero_grad(set_to_none=True)
        out = model(images, texts)
        loss = ClipLoss()(**out, output_dict=True)["total_loss"]
        loss.backward()
        opt.step()
        losses.append(float(loss))
    with torch.no_grad():
        model(images, texts)
    checked = 0
    split = 0
    for prefix, eng in (("visual.", model.visual._engine), ("", model._text_engine)):
        params = dict(model.named_parameters())
        for name, ent in eng._shadow.items():
            if "#" in name:          # `<in_proj_weight>#q` / `#kv`: row ranges of the last block's packed in_proj (split GEMMs)
                base, part = name.split("#")
                full = params[prefix + base].detach()
                p = full[:full.shape[0] // 3] if part == "q" else full[full.shape[0] // 3:]
                split += 1
            else:
                p = params[prefix + name]
            w = p.detach().view(p.shape[0], -1) if p.ndim != 2 else p.detach()
            if ent[0].shape == w.shape:
                assert torch.equal(ent[0], w.to(torch.bfloat16)), name
                assert torch.equal(ent[1], w.t().contiguous().to(torch.bfloat16)), name
                checked += 1
    assert checked >= 8 and split == 4      # (q and k | v copies of both towers' last blocks)
    assert losses[2] < losses[0]            # the same batch three times at lr 1e-2: the loss must move


def test_grads_are_arena_views_and_hook_fires(golden_dir):
    """autograd must install the returned gradient views as .grad without a deep copy (GradSync all-reduces the
    flat arenas in place), and each tower must announce every element of its arena exactly once per backward (as a few
    ranges, the arena's tail first)."""
    z = _load(golden_dir, "tiny_clip.npz")
    sd = {k[3:]: _t(v) for k, v in z.items() if k.startswith("sd/")}
    model = build("ViT-tiny-test", sd, "fp32")
    seen = []
    model.visual._engine.grad_ready_hook = lambda arena: seen.append(("v", arena.data_ptr(), arena.numel()))
    model._text_engine.grad_ready_hook = lambda arena: seen.append(("t", arena.data_ptr(), arena.numel()))
    model.zero_grad(set_to_none=True)
    out = model(_t(z["image"]).to(DEV), _t(z["text"]).to(DEV))
    ClipLoss()(**out).backward()
    spans = {}
    for key, eng in (("v", model.visual._engine), ("t", model._text_engine)):
        base, numel = eng._arena.data_ptr(), eng._arena.numel()
        mine = sorted((lo, n) for k, lo, n in seen if k == key)
        assert mine and mine[0][0] == base
        end = base
        for lo, n in mine:
            assert lo == end, "early ranges must tile the arena without gap or overlap"
            end = lo + 4 * n
        assert end == base + 4 * numel
        spans[key] = (base, end)
    for name, p in model.named_parameters():
        if name == "logit_scale":
            continue
        lo, hi = spans["v" if name.startswith("visual.") else "t"]
        assert lo <= p.grad.data_ptr() < hi, f"{name}: .grad was deep-copied out of the arena"


# ------------------------------------------------------------------ ColClipLoss ("next" row 8f-2)
def test_colclip_loss_golden_fp32(golden_dir):
    """ColClipLoss through the HIP kernels vs the reference's own loss.py (fixture): losses and every gradient."""
    from colxlip_amd.loss import ColClipLoss, compute_colbert_similarity
    z = _load(golden_dir, "colclip_loss.npz")
    for tag in ("a", "b"):
        base = [_t(z[f"{tag}/{k}"]).to(DEV) for k in ("image_features", "text_features", "token_image_features",
                                                      "token_text_features", "log_logit_scale")]
        sim = compute_colbert_similarity(base[2], base[3]) * base[4].exp()
        assert float((sim.cpu() - _t(z[f"{tag}/logits_per_text_token"])).abs().max()) < 1e-4
        for alpha in (0.5, 0.2):
            fi, ft, ti, tt, lls = [t.clone().requires_grad_(True) for t in base]
            res = ColClipLoss(alpha=alpha)(image_features=fi, text_features=ft, token_image_features=ti,
                                           token_text_features=tt, logit_scale=lls.exp(), output_dict=True)
            res["total_loss"].backward()
            k = f"{tag}/alpha{alpha}"
            assert abs(float(res["global_contrastive_loss"]) - float(z[f"{k}/global_loss"])) < 1e-4
            assert abs(float(res["token_contrastive_loss"]) - float(z[f"{k}/token_loss"])) < 1e-4
            assert abs(float(res["total_loss"]) - float(z[f"{k}/total_loss"])) < 1e-4
            for leaf, name in ((fi, "grad_image"), (ft, "grad_text"), (ti, "grad_token_image"), (tt, "grad_token_text"),
                               (lls, "grad_log_logit_scale")):
                ref = _t(z[f"{k}/{name}"])
                err = float((leaf.grad.cpu() - ref).abs().max())
                assert err < 1e-5 + 1e-3 * float(ref.abs().max()), (k, name, err)


def test_colclip_loss_bf16_chunked():
    """bf16 token features: MFMA NT/TN GEMM path, several text chunks, vs the fp32 path on the same (bf16-rounded) data."""
    from colxlip_amd import loss as LS, ops
    torch.manual_seed(3)
    n, nt, nq, e = 16, 77, 49, 64
    ti = torch.nn.functional.normalize(torch.randn(n, nq, e, device=DEV), dim=-1).bfloat16()
    tt = torch.nn.functional.normalize(torch.randn(n, nt, e, device=DEV), dim=-1).bfloat16()
    g = torch.randn(n, n, device=DEV)
    old = ops.MAXSIM_GENERAL_BYTES
    ops.MAXSIM_GENERAL_BYTES = 8 * nt * n * nq * 2                # 8 text samples per chunk -> 2 chunks
    try:
        a, b = ti.clone().requires_grad_(True), tt.clone().requires_grad_(True)
        out = LS.compute_colbert_similarity(a, b)
        out.backward(g)
    finally:
        ops.MAXSIM_GENERAL_BYTES = old
    a32, b32 = ti.float().requires_grad_(True), tt.float().requires_grad_(True)
    ref = LS.compute_colbert_similarity(a32, b32)
    ref.backward(g)
    assert float((out - ref).abs().max()) < 2e-2
    # arg-max ties can differ between bf16 and fp32 products on a few (m,n,k): compare gradients in norm
    for got, want in ((a.grad.float(), a32.grad), (b.grad.float(), b32.grad)):
        assert float((got - want).norm() / want.norm()) < 0.12


@pytest.mark.parametrize("ni,q,nt,n,e", [(8, 196, 8, 77, 512), (5, 64, 6, 9, 128), (4, 100, 4, 7, 256), (16, 256, 16, 77, 128),
                                          (4, 576, 3, 20, 128)])
def test_maxsim_fused_vs_torch(ni, q, nt, n, e, monkeypatch):
    """The fused MaxSim (csrc/gemm_nt_maxsim.h + csrc/colbert.hip; bf16 tokens, >= 64 tokens per image: ViT-B-16-colxlip has 196)
    against the reference's arithmetic (loss.py:20-46) in fp32 on the same bf16 values, forward and both gradients.  The text
    batch is built like ColXLIP's (every position at / behind a per-sample EOT is ONE vector: those rows are folded into one
    weighted row inside), with one sample of exact-zero masked rows (the reference's non-zero count) and one sample without any
    duplicate.  Image-token counts that are not multiples of 64 or of 4 put image boundaries inside a wave's 64 columns and
    inside an accumulator quad.  Also against the unfused path, which writes the similarity matrix."""
    from colxlip_amd import loss as LS
    g = torch.Generator().manual_seed(100 + q)
    ti = torch.nn.functional.normalize(torch.randn(ni, q, e, generator=g), dim=-1)
    tt = torch.nn.functional.normalize(torch.randn(nt, n, e, generator=g), dim=-1)
    tail = torch.nn.functional.normalize(torch.randn(e, generator=g), dim=-1)
    for m in range(nt):
        eot = 2 + (5 * m) % (n - 2)
        if m == 1:
            tt[m, eot:] = 0.0                      # exact-zero rows: similarity 0, not counted by the masked mean
        elif m != 2:                               # sample 2 keeps distinct rows to the end
            tt[m, eot:] = tail
    a = ti.to(DEV).bfloat16().requires_grad_(True)
    b = tt.to(DEV).bfloat16().requires_grad_(True)
    assert LS._MaxSimFused.applies(a, b)
    out = LS.compute_colbert_similarity(a, b)
    gout = torch.randn(nt, ni, generator=g).to(DEV)
    out.backward(gout)
    a32 = a.detach().float().requires_grad_(True)
    b32 = b.detach().float().requires_grad_(True)
    sim = torch.einsum('mnd,kqd->mknq', b32, a32)
    mx = sim.max(dim=3)[0]
    nz = (mx != 0).float()
    ref = mx.sum(-1) / (nz.sum(-1) + 1e-8)          # reference loss.py:37-44: the SUM runs over every position, the count over non-zero maxima
    ref.backward(gout)
    assert float((out - ref).abs().max()) < 2e-5, float((out - ref).abs().max())
    for got, want, name in ((a.grad.float(), a32.grad, "image tokens"), (b.grad.float(), b32.grad, "text tokens")):
        rel = float((got - want).norm() / want.norm())
        assert rel < 6e-3, (name, rel)             # coefficients of d(S) and the gradients themselves are rounded to bf16
        cos = float((got * want).sum() / (got.norm() * want.norm()))
        assert cos > 0.9999, (name, cos)
    # every position of a folded tail receives the representative's gradient; masked zero rows still pass one to their arg-max
    eot0 = 2
    assert torch.equal(b.grad[0, eot0], b.grad[0, n - 1]) and float(b.grad[0, eot0].float().norm()) > 0
    assert float(b.grad[1, n - 1].float().norm()) > 0
    # the unfused path (similarity matrix written, reduced by a second kernel) on the same inputs
    monkeypatch.setenv("CLIPX_MAXSIM_FUSED", "0")
    a2 = a.detach().clone().requires_grad_(True)
    b2 = b.detach().clone().requires_grad_(True)
    assert not LS._MaxSimFused.applies(a2, b2)
    if q <= 255 and (ni * q) % 8 == 0 and (nt * n) % 8 == 0 and nt % 8 == 0:
        out2 = LS.compute_colbert_similarity(a2, b2)
        assert float((out2 - out).abs().max()) < 2e-2       # there S is rounded to bf16 before the max


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_colxlip_model_vs_oracle(precision):
    """ColXLIP (token heads, EOT masking, MaxSim loss) on the width-128 model vs the CPU oracle's restatement of reference
    model.py:455-687.  The reference class itself cannot be imported here (open_clip is absent): "parity unpinned" for
    the wrapper, its loss is pinned by tests above."""
    from colxlip_amd.loss import ColClipLoss
    cfg = O.ClipCfg(embed_dim=64, image_size=64, patch_size=16, vision_width=128, vision_layers=2,
                    context_length=77, vocab_size=1024, text_width=128, text_heads=2, text_layers=2)
    sd = O.perturb_state_dict(O.init_state_dict(cfg, seed=3), seed=4)
    sd.update(O.perturb_state_dict(O.init_colxlip_heads(cfg, seed=5), seed=6))
    image, text = O.synthetic_batch(cfg, 8, seed=21)
    ref_out, ref_res, ref_grads = O.colxlip_loss_and_grads(sd, image, text, cfg, alpha=0.4)
    model = build("ViT-small-test-colxlip", sd, precision)
    model.train()
    model.zero_grad(set_to_none=True)
    out = model(image.to(DEV), text.to(DEV))
    res = ColClipLoss(alpha=0.4)(**out, output_dict=True)
    res["total_loss"].backward()
    ftol, ltol, gtol = (2e-5, 2e-5, 3e-3) if precision == "fp32" else (4e-2, 6e-2, 0.2)
    for k in ("image_features", "text_features", "token_image_features", "token_text_features"):
        assert float((out[k].detach().float().cpu() - ref_out[k]).abs().max()) < ftol, k
    for k in ("global_contrastive_loss", "token_contrastive_loss", "total_loss"):
        assert abs(float(res[k]) - float(ref_res[k])) < ltol, k
    grads = {k: p.grad.detach().float().cpu() for k, p in model.named_parameters() if p.grad is not None}
    for k in sd:
        ref = ref_grads[k]
        if float(ref.norm()) > 1e-4:
            rel = float((grads[k] - ref).norm() / (ref.norm() + 1e-8))
            assert rel < gtol, (k, rel)


def test_compute_retrieval_matches_argsort_reference():
    """Retrieval metrics: rank-count kernel vs a literal restatement of reference train.py:457-508 (argsort
    per row, search the ground truth; 5 captions per image)."""
    import numpy as np
    from colxlip_amd.train import compute_retrieval, similarity_matrix
    torch.manual_seed(0)
    n_img, per = 40, 5
    n_txt = n_img * per
    fi = torch.nn.functional.normalize(torch.randn(n_img, 32, device=DEV), dim=-1)
    ft = torch.nn.functional.normalize(torch.randn(n_txt, 32, device=DEV) + 0.7 * fi.repeat_interleave(per, 0), dim=-1)
    txt2img = {c: c // per for c in range(n_txt)}
    img2txt = {i: list(range(i * per, (i + 1) * per)) for i in range(n_img)}
    sim = similarity_matrix(fi, ft)
    assert float((sim - fi @ ft.t()).abs().max()) < 1e-5
    got = compute_retrieval(sim, txt2img, img2txt)

    s = sim.cpu()
    t2i_ranks = torch.zeros(n_txt)
    for index, score in enumerate(s.t()):
        inds = torch.argsort(score, descending=True)
        t2i_ranks[index] = torch.where(inds == txt2img[index])[0][0]
    i2t_ranks = torch.zeros(n_img)
    for index, score in enumerate(s):
        inds = torch.argsort(score, descending=True)
        i2t_ranks[index] = min(int(torch.where(inds == i)[0][0]) for i in img2txt[index])
    for prefix, ranks in (("text_to_image", t2i_ranks), ("image_to_text", i2t_ranks)):
        assert abs(got[f"{prefix}_R@1"] - len(torch.where(ranks < 1)[0]) / len(ranks)) < 1e-9
        assert abs(got[f"{prefix}_R@5"] - len(torch.where(ranks < 5)[0]) / len(ranks)) < 1e-9
        assert abs(got[f"{prefix}_R@10"] - len(torch.where(ranks < 10)[0]) / len(ranks)) < 1e-9
        assert abs(got[f"{prefix}_mean_rank"] - (ranks.mean().item() + 1)) < 1e-4
        assert got[f"{prefix}_median_rank"] == np.floor(np.median(ranks.numpy())) + 1


def test_convert_weights_to_lp_on_device(golden_dir):
    """SURVEY a2 on the GPU: after `convert_weights_to_lp(model, bfloat16)` a parity-mode model (a) holds the values of the
    reference's own run of that function (tests/golden/lp_convert.npz), (b) computes in bf16 -- its step equals, bit for bit,
    the step of a `--precision bf16` model loaded with those values (the operand copies are refreshed: `copy_` bumped the
    versions), and (c) agrees with the fp32 oracle run ON the converted values within the bf16 tolerances."""
    from colxlip_amd import convert_weights_to_lp
    z = _load(golden_dir, "lp_convert.npz")
    sd = O.perturb_state_dict(O.init_state_dict(O.TINY, seed=0), seed=1)
    image, text = O.synthetic_batch(O.TINY, 8, seed=1234)
    model = build("ViT-tiny-test", sd, "fp32")
    run_step(model, image, text)                                  # fp32 step first: any cached state predates the conversion
    convert_weights_to_lp(model, dtype=torch.bfloat16)
    after = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    for name in z["all_names"]:
        assert torch.equal(after[str(name)], _t(z["after/" + str(name)])), name
    out_c, loss_c, grads_c = run_step(model, image, text)
    twin = build("ViT-tiny-test", after, "bf16")
    out_t, loss_t, grads_t = run_step(twin, image, text)
    assert loss_c == loss_t and torch.equal(out_c["image_features"], out_t["image_features"])
    for k in grads_c:       # equal up to the summation order of the fp32 atomics in the embedding / LayerNorm reductions
        assert float((grads_c[k] - grads_t[k]).abs().max()) <= 1e-5 * float(grads_t[k].abs().max()) + 1e-9, k
    ref_out, ref_loss, _ = O.loss_and_grads(after, image, text, O.TINY)
    assert float((out_c["image_features"] * ref_out["image_features"]).sum(-1).min()) > 0.999
    assert abs(loss_c - float(ref_loss)) < 5e-2
