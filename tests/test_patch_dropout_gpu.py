"""Patch dropout on the MI355X (csrc/patch_dropout.hip + the image tower's per-forward sequence length): the device mask draw, the
gathered patchify and assemble against the dense kernels bit for bit, the assemble backward against a float64 scatter-add, the
model against the reference's PatchDropout (tests/golden/patch_dropout.npz, rng="torch"), inactive paths bit-identical to a model
without dropout, the mask's lifetime (backward, checkpoint recompute, fresh draws) and `main --force-patch-dropout`."""
import logging
import math
import os

import numpy as np
import pytest
import torch

from colxlip_amd import ClipLoss, create_model_and_transforms, ops
from colxlip_amd.model import PatchDropout

pytestmark = pytest.mark.gpu
DEV = "cuda"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "patch_dropout.npz")


def _torch_index(batch, G2, keep, seed):
    """the reference's draw: topk order, not sorted"""
    g = torch.Generator().manual_seed(seed)
    return torch.randn(batch, G2, generator=g).topk(keep, dim=-1).indices.to(torch.int32).to(DEV)


# ------------------------------------------------------------------ kernels
@pytest.mark.parametrize("G2,keep", [(4, 1), (4, 2), (16, 8), (49, 24), (196, 98), (196, 1), (576, 144), (1024, 1000), (20, 20)])
def test_keep_index_is_a_sorted_subset(G2, keep):
    b = 96
    idx = ops.patch_keep_index(b, G2, keep, 12345, DEV)
    assert idx.shape == (b, keep) and idx.dtype == torch.int32
    i = idx.long().cpu()
    assert int(i.min()) >= 0 and int(i.max()) < G2
    if keep > 1:
        assert bool((i[:, 1:] > i[:, :-1]).all())                        # strictly ascending: distinct
    assert torch.equal(idx, ops.patch_keep_index(b, G2, keep, 12345, DEV))
    # a function of (key, sample) only: a smaller batch draws the same first rows
    assert torch.equal(ops.patch_keep_index(7, G2, keep, 12345, DEV), idx[:7])
    if keep < G2 and math.comb(G2, keep) > 10 ** 6:
        assert not torch.equal(ops.patch_keep_index(b, G2, keep, 12346, DEV), idx)
        other = ops.patch_keep_index(b, G2, keep, 12346, DEV).cpu()
        assert sum(not torch.equal(other[s], i[s]) for s in range(b)) > b // 2
        assert len({tuple(r.tolist()) for r in i}) > b // 2               # samples draw different sets


@pytest.mark.parametrize("G2", [4, 49, 196, 576])
def test_keep_index_is_uniform(G2):
    b = 8192
    keep = PatchDropout(0.5).num_keep(G2)
    idx = ops.patch_keep_index(b, G2, keep, 987654321, DEV).long()
    freq = torch.bincount(idx.reshape(-1), minlength=G2).double().cpu() / b
    q = keep / G2
    sigma = math.sqrt(q * (1 - q) / b)
    assert float((freq - q).abs().max()) <= 6 * sigma, (float((freq - q).abs().max()), sigma)


def test_keep_index_checks_its_arguments():
    with pytest.raises(RuntimeError):
        ops.patch_keep_index(2, 1025, 10, 1, DEV)
    with pytest.raises(RuntimeError):
        ops.patch_keep_index(2, 16, 17, 1, DEV)
    assert ops.patch_keep_index(0, 16, 8, 1, DEV).shape == (0, 8)


@pytest.mark.parametrize("img_dt,dt", [(torch.float32, torch.float32), (torch.float32, torch.bfloat16),
                                       (torch.bfloat16, torch.bfloat16), (torch.bfloat16, torch.float32)])
@pytest.mark.parametrize("size,P,Kp", [(64, 16, 768), (224, 32, 3072), (56, 14, 640), (56, 14, 588)])
def test_patchify_keep_equals_gathered_patchify(img_dt, dt, size, P, Kp):
    b = 5
    G2 = (size // P) ** 2
    keep = max(1, G2 // 2)
    image = torch.randn(b, 3, size, size, device=DEV).to(img_dt)
    dense = ops.patchify(image, P, Kp, dt).view(b, G2, Kp)
    for idx in (_torch_index(b, G2, keep, 3), ops.patch_keep_index(b, G2, keep, 99, DEV)):
        got = ops.patchify_keep(image, P, Kp, dt, idx).view(b, keep, Kp)
        want = torch.gather(dense, 1, idx.long().unsqueeze(-1).expand(b, keep, Kp))
        assert torch.equal(got, want)


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("G2,keep,width", [(16, 8, 128), (49, 24, 768), (196, 98, 768), (196, 1, 64)])
def test_assemble_keep_equals_dense_rows(dt, G2, keep, width):
    b = 6
    cls = torch.randn(width, device=DEV)
    pos = torch.randn(G2 + 1, width, device=DEV)
    tok_dense = torch.randn(b * G2, width, device=DEV).to(dt)
    dense = ops.vision_assemble(tok_dense, cls, pos, b, G2 + 1).view(b, G2 + 1, width)
    idx = _torch_index(b, G2, keep, 5)
    tok = torch.gather(tok_dense.view(b, G2, width), 1, idx.long().unsqueeze(-1).expand(b, keep, width)).reshape(b * keep, width)
    got = ops.vision_assemble_keep(tok.contiguous(), cls, pos, idx, G2).view(b, keep + 1, width)
    assert torch.equal(got[:, 0], dense[:, 0])
    want = torch.gather(dense[:, 1:], 1, idx.long().unsqueeze(-1).expand(b, keep, width))
    assert torch.equal(got[:, 1:], want)


def _assemble_bwd_f64(dx0, idx, G2, dpos_old, dcls_old, beta):
    b, keep = idx.shape
    width = dx0.shape[-1]
    d = dx0.double().view(b, keep + 1, width)
    dpos = beta * dpos_old.double()
    dpos[0] += d[:, 0].sum(0)
    dpos[1:].index_add_(0, idx.long().reshape(-1), d[:, 1:].reshape(-1, width))
    dcls = beta * dcls_old.double() + d[:, 0].sum(0)
    scale = torch.zeros(G2 + 1, width, dtype=torch.float64, device=dx0.device)
    scale[0] += d[:, 0].abs().sum(0)
    scale[1:].index_add_(0, idx.long().reshape(-1), d[:, 1:].abs().reshape(-1, width))
    return dpos, dcls, scale + (beta * dpos_old.double()).abs()


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("b,G2,keep,width", [(8, 16, 8, 128), (100, 49, 24, 768), (300, 196, 98, 256), (3, 576, 5, 64)])
@pytest.mark.parametrize("beta", [0.0, 1.0, 0.5])
@pytest.mark.parametrize("order", ["topk", "device"])
def test_assemble_keep_bwd(dt, b, G2, keep, width, beta, order):
    idx = _torch_index(b, G2, keep, 11) if order == "topk" else ops.patch_keep_index(b, G2, keep, 7, DEV)
    dx0 = torch.randn(b * (keep + 1), width, device=DEV).to(dt)
    dpos_old = torch.randn(G2 + 1, width, device=DEV)
    dcls_old = torch.randn(width, device=DEV)
    runs = []
    for _ in range(2):
        dpos, dcls = dpos_old.clone(), dcls_old.clone()
        dtok = ops.vision_assemble_keep_bwd(dx0, idx, G2, dpos, dcls, beta)
        runs.append((dtok, dpos, dcls))
    dtok, dpos, dcls = runs[0]
    for a, c in zip(runs[0], runs[1]):
        assert torch.equal(a, c)                                          # the same bits every run
    assert torch.equal(dtok, dx0.view(b, keep + 1, width)[:, 1:].reshape(b * keep, width))
    want_pos, want_cls, scale = _assemble_bwd_f64(dx0, idx, G2, dpos_old, dcls_old, beta)
    assert bool(((dpos.double() - want_pos).abs() <= 1e-6 * scale + 1e-30).all())
    assert bool(((dcls.double() - want_cls).abs() <= 1e-6 * scale[0] + 1e-30).all())
    kept = torch.zeros(G2, dtype=torch.bool, device=DEV)
    kept[idx.long().reshape(-1)] = True
    never = torch.nonzero(~kept).reshape(-1) + 1
    if never.numel():
        assert torch.equal(dpos[never], beta * dpos_old[never] if beta != 0.0 else torch.zeros_like(dpos_old[never]))


@pytest.mark.parametrize("beta", [0.0, 1.0, 0.5])
def test_assemble_keep_bwd_empty_batch(beta):
    G2, width = 49, 128
    dpos_old, dcls_old = torch.randn(G2 + 1, width, device=DEV), torch.randn(width, device=DEV)
    dpos, dcls = dpos_old.clone(), dcls_old.clone()
    dtok = ops.vision_assemble_keep_bwd(torch.empty(0, width, device=DEV), torch.empty(0, 24, dtype=torch.int32, device=DEV), G2,
                                        dpos, dcls, beta)
    torch.cuda.synchronize()
    assert dtok.shape == (0, width)
    assert torch.equal(dpos, dpos_old * beta) and torch.equal(dcls, dcls_old * beta)


# ------------------------------------------------------------------ model
def _fixture(tag):
    z = np.load(GOLDEN)
    return {k.split("/", 1)[1]: z[k] for k in z.files if k.startswith(tag + "/")}


def _grad_sample_index(numel, n):
    if numel <= n:
        return torch.arange(numel)
    return (torch.arange(n, dtype=torch.int64) * numel) // n


_MODEL = {"small": "ViT-small-test", "b16": "ViT-B-16"}


def _fixture_inputs(tag, z):
    import json
    from oracle import clip_oracle as O
    name = _MODEL[tag.split("_")[0]]
    if name == "ViT-small-test":
        path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "model_configs", name + ".json")
    else:
        path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "colxlip_amd", "model_configs", name + ".json")
    with open(path) as f:
        cfg = O.ClipCfg.from_model_json(json.load(f))
    sd = O.perturb_state_dict(O.init_state_dict(cfg, seed=0), seed=1)
    image, text = O.synthetic_batch(cfg, int(z["batch"]), seed=1234)
    assert np.allclose([float(sd[k].double().sum()) for k in sorted(sd.keys())], z["sd_checksum"], rtol=1e-9, atol=1e-9)
    assert np.allclose([float(image.double().sum()), float(text.double().sum())], z["batch_checksum"], rtol=1e-9, atol=1e-9)
    return name, sd, image, text


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("tag", ["small_p50", "small_p75", "b16_p50"])
def test_parity_with_reference_patch_dropout(tag, precision):
    z = _fixture(tag)
    name, sd, image, text = _fixture_inputs(tag, z)
    model, _, _ = create_model_and_transforms(name, precision=precision, device=DEV, output_dict=True,
                                              force_patch_dropout=float(z["prob"]))
    model.load_state_dict(sd)
    model.visual.patch_dropout.rng = "torch"
    model.train()
    image = image.to(DEV)
    torch.manual_seed(int(z["seed"]))
    out = model(image.bfloat16() if precision == "bf16" else image, text.to(DEV))
    assert np.array_equal(model.visual.patch_dropout.last_keep_index.cpu().numpy(), z["keep_index"])
    loss = ClipLoss()(**out)
    loss.backward()
    loss = float(loss.detach())
    grads = {k: p.grad.detach().float().cpu() for k, p in model.named_parameters()}
    names = [str(n) for n in z["grad_names"]]
    assert sorted(names) == sorted(grads)
    fi, ft = out["image_features"].detach().float().cpu(), out["text_features"].detach().float().cpu()
    want_fi, want_ft = torch.from_numpy(z["image_features"]), torch.from_numpy(z["text_features"])
    full = name != "ViT-small-test"
    if precision == "fp32":
        # the bars of tests/test_siglip_gpu.py; full-size towers (12 blocks of width 768) get test_configs_gpu.py's fp32 bars
        ftol, gtol = (1e-4, 5e-3) if full else (1e-5, 2e-3)
        assert float((fi - want_fi).abs().max()) < ftol
        assert float((ft - want_ft).abs().max()) < ftol
        assert abs(loss - float(z["loss"])) < (1e-3 if full else 1e-5 * abs(float(z["loss"])))
        n_s = z["grad_sample"].shape[1]
        for i, k in enumerate(names):
            g = grads[k].reshape(-1)
            got = g[_grad_sample_index(g.numel(), n_s)]
            want = torch.from_numpy(z["grad_sample"][i][:got.numel()]).float()
            scale = float(z["grad_maxabs"][i]) + 1e-8
            assert float((got - want).abs().max()) < (1e-3 if full else 2e-3) * scale, k
            assert abs(float(g.double().norm()) - float(z["grad_norms"][i])) < gtol * float(z["grad_norms"][i]) + 1e-8, k
    else:
        assert float((fi * want_fi).sum(-1).min()) > 0.999
        assert float((ft * want_ft).sum(-1).min()) > 0.999
        assert abs(loss - float(z["loss"])) < 2e-2
        gmax = float(np.max(z["grad_norms"]))
        for i, k in enumerate(names):
            want = float(z["grad_norms"][i])
            got = float(grads[k].double().norm())
            if k != "logit_scale" and want > 1e-7:
                assert max(0.0, abs(got - want) - 3e-5 * gmax) / want < 0.03, (k, got, want)


def _build(p=None, precision="fp32", name="ViT-small-test", seed=0):
    torch.manual_seed(seed)
    kw = {} if p is None else {"force_patch_dropout": p}
    model, _, _ = create_model_and_transforms(name, precision=precision, device=DEV, output_dict=True, **kw)
    return model


def _batch(model, b=8, seed=1234, dtype=torch.float32):
    from colxlip_amd.data import synthetic_batch
    images, texts = synthetic_batch(b, model.visual.image_size, model.context_length, model.vocab_size, seed=seed, device=DEV,
                                    image_dtype=dtype)
    return images, texts[:, 0].contiguous()


def _step(model, image, text, seed=None):
    for p in model.parameters():
        p.grad = None
    if seed is not None:
        torch.manual_seed(seed)
    out = model(image, text)
    loss = ClipLoss()(**out)
    loss.backward()
    torch.cuda.synchronize()
    return out, loss.detach(), {k: p.grad.detach().clone() for k, p in model.named_parameters()}


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_dropout_zero_is_bit_identical_to_no_dropout(precision):
    m0 = _build(None, precision)
    m1 = _build(0.0, precision)
    m1.load_state_dict(m0.state_dict())
    m0.train()
    m1.train()
    image, text = _batch(m0, dtype=torch.bfloat16 if precision == "bf16" else torch.float32)
    o0, l0, g0 = _step(m0, image, text, seed=1)
    o1, l1, g1 = _step(m1, image, text, seed=1)
    assert m1.visual.patch_dropout.last_keep_index is None
    assert torch.equal(o0["image_features"], o1["image_features"]) and torch.equal(l0, l1)
    for k in g0:
        assert torch.equal(g0[k], g1[k]), k


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_eval_mode_does_not_drop(precision):
    m0 = _build(None, precision)
    m5 = _build(0.5, precision)
    m5.load_state_dict(m0.state_dict())
    m0.eval()
    m5.eval()
    image, text = _batch(m0, dtype=torch.bfloat16 if precision == "bf16" else torch.float32)
    with torch.no_grad():
        a, b = m0(image, text), m5(image, text)
    assert m5.visual.patch_dropout.last_keep_index is None
    assert torch.equal(a["image_features"], b["image_features"])
    m5.train()
    with torch.no_grad():
        c = m5(image, text)
    assert m5.visual.patch_dropout.last_keep_index is not None
    assert not torch.equal(a["image_features"], c["image_features"])


def test_evaluate_runs_without_dropping(tmp_path):
    from colxlip_amd.data import synthetic_retrieval_split
    from colxlip_amd.params import parse_args
    from colxlip_amd.train import evaluate
    m0 = _build(None)
    m5 = _build(0.5)
    m5.load_state_dict(m0.state_dict())
    m0.train()
    m5.train()
    split = synthetic_retrieval_split(24, 5, 64, 77, 1024, seed=99, device=DEV, batch_size=7)
    a = parse_args(["--model", "ViT-small-test", "--dataset-type", "synthetic", "--precision", "fp32", "--batch-size", "8",
                    "--epochs", "1"])
    a.rank, a.local_rank, a.world_size, a.distributed, a.device = 0, 0, 1, False, "cuda"
    a.save_logs, a.wandb = False, False
    r0 = evaluate(m0, {"retrieval_coco": split}, 1, a)
    r5 = evaluate(m5, {"retrieval_coco": split}, 1, a)
    assert m5.training and m5.visual.patch_dropout.last_keep_index is None
    assert r0 and r0 == r5


@pytest.mark.parametrize("keep_env", ["0", "1", ""])
def test_checkpoint_recompute_uses_the_forward_mask(keep_env, monkeypatch):
    model = _build(0.5)
    model.train()
    image, text = _batch(model)
    _, l_ref, g_ref = _step(model, image, text, seed=21)
    idx_ref = model.visual.patch_dropout.last_keep_index.clone()
    monkeypatch.setenv("CLIPX_CKPT_KEEP", keep_env)
    model.set_grad_checkpointing(True)
    for e in (model.visual._engine, model._text_engine):
        e._keep_cache = None
    _, l_ck, g_ck = _step(model, image, text, seed=21)
    assert torch.equal(model.visual.patch_dropout.last_keep_index, idx_ref)
    assert torch.allclose(l_ck, l_ref, rtol=1e-5)
    for k in g_ref:
        assert torch.allclose(g_ck[k], g_ref[k], rtol=1e-4, atol=1e-7), k


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_same_seed_same_bits_and_fresh_masks(precision):
    model = _build(0.5, precision)
    model.train()
    image, text = _batch(model, dtype=torch.bfloat16 if precision == "bf16" else torch.float32)
    pd = model.visual.patch_dropout
    o1, l1, g1 = _step(model, image, text, seed=5)
    i1 = pd.last_keep_index.clone()
    o2, l2, g2 = _step(model, image, text, seed=5)
    assert torch.equal(pd.last_keep_index, i1)
    assert torch.equal(o1["image_features"], o2["image_features"]) and torch.equal(l1, l2)
    for k in g1:
        assert torch.equal(g1[k], g2[k]), k
    # consecutive training forwards draw new masks, a no_grad training forward (the accumulation path's caching pass) included
    masks = [i1]
    with torch.no_grad():
        model(image, text)
    masks.append(pd.last_keep_index.clone())
    _step(model, image, text)
    masks.append(pd.last_keep_index.clone())
    for a in range(len(masks)):
        for b in range(a + 1, len(masks)):
            assert not torch.equal(masks[a], masks[b])
    # the gradient reaches only positional rows some sample kept (plus the class token's row)
    g_pos = g1["visual.positional_embedding"]
    kept = torch.zeros(g_pos.shape[0], dtype=torch.bool, device=DEV)
    kept[0] = True
    kept[i1.long().reshape(-1) + 1] = True
    assert bool((g_pos[~kept] == 0).all()) and bool((g_pos[kept].abs().sum(-1) > 0).all())


def test_fp8_mfma_step_with_patch_dropout():
    model = _build(0.5, "fp8_mfma", name="ViT-B-32")
    model.train()
    image, text = _batch(model, b=8, dtype=torch.bfloat16)
    _, loss, grads = _step(model, image, text, seed=3)
    assert model.visual.patch_dropout.last_keep_index.shape == (8, 24)
    assert math.isfinite(float(loss))
    for k, g in grads.items():
        assert bool(torch.isfinite(g).all()), k


def test_main_trains_with_patch_dropout(tmp_path, caplog):
    from colxlip_amd.main import main
    steps = 4
    argv = ["--model", "ViT-small-test", "--dataset-type", "synthetic", "--precision", "fp32", "--batch-size", "8",
            "--force-patch-dropout", "0.5", "--lr", "1e-3", "--wd", "0.1", "--lr-scheduler", "const", "--warmup", "1",
            "--epochs", "1", "--train-num-samples", str(8 * steps), "--logs-dir", str(tmp_path), "--name", "pd",
            "--log-every-n-steps", "1", "--seed", "3", "--retrieval-coco", "--val-num-samples", "16"]
    with caplog.at_level(logging.INFO):
        assert main(argv) == 0
    msgs = [r.getMessage() for r in caplog.records]
    lines = [m for m in msgs if m.startswith("Train Epoch")]
    assert len(lines) == steps
    vals = [float(l.split("Total_loss: ")[1].split()[0]) for l in lines]
    assert all(math.isfinite(v) and v > 0 for v in vals)
    assert any(m.startswith("Eval Epoch: 1 ") for m in msgs)
