"""SigLipLoss on the MI355X (csrc/loss_sigmoid.hip): the fused and materialising kernels against the reference's own SigLipLoss
(tests/golden/siglip_loss.npz, written by make_golden_siglip.py), a float64 evaluation at N = 4096, run-to-run bit identity,
the negatives-only and non-square blocks, the no_grad walk, the full CLIP model (siglip_tiny.npz) and `main --siglip`."""
import logging
import math
import os

import numpy as np
import pytest
import torch

from colxlip_amd import SigLipLoss, create_model_and_transforms, ops
from colxlip_amd.loss import _SigmoidLoss

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load(golden_dir, name):
    z = np.load(os.path.join(golden_dir, name), allow_pickle=False)
    return {k: z[k] for k in z.files}


def _t(a):
    return torch.from_numpy(np.asarray(a))


def _leaves(fi, ft, log_scale, bias):
    fi = _t(fi).to(DEV).float().requires_grad_(True)
    ft = _t(ft).to(DEV).float().requires_grad_(True)
    ls = _t(log_scale).to(DEV).float().reshape(()).requires_grad_(True)
    lb = _t(bias).to(DEV).float().reshape(()).requires_grad_(True)
    return fi, ft, ls, lb


def _step(fi, ft, ls, lb, pos_off=0):
    loss = _SigmoidLoss.apply(fi, ft, ls.exp(), lb, pos_off, True)
    loss.backward()
    return loss.detach(), fi.grad.detach(), ft.grad.detach(), ls.grad.detach(), lb.grad.detach()


def _f64(fi, ft, s, beta, pos_off):
    """the formula in float64 on the device: loss, dA, dB, d(log scale), d(bias)"""
    A, B = fi.double(), ft.double()
    dot = A @ B.T
    z = s * dot + beta
    y = -torch.ones_like(z)
    if pos_off >= 0:
        idx = torch.arange(A.shape[0], device=A.device)
        y[idx, idx + pos_off] = 1.0
    r = A.shape[0]
    loss = torch.nn.functional.softplus(-y * z).sum() / r
    dz = -y * torch.sigmoid(-y * z) / r
    return loss, s * dz @ B, s * dz.T @ A, s * (dz * dot).sum(), dz.sum()


@pytest.mark.parametrize("tag", ["a", "b", "c", "d"])
def test_kernels_vs_reference_fixture(golden_dir, tag):
    """a, d: fused (E = 64; d has s = 100, beta = -10, |z| > 88); b: fused E = 512, b = 100; c: E = 48, the materialising path"""
    z = _load(golden_dir, "siglip_loss.npz")
    fi, ft, ls, lb = _leaves(z[f"{tag}/image_features"], z[f"{tag}/text_features"], z[f"{tag}/log_logit_scale"],
                             z[f"{tag}/logit_bias"])
    assert (fi.shape[1] in ops.FUSED_CE_DIMS) == (tag != "c")
    loss, gi, gt, gs, gb = _step(fi, ft, ls, lb)
    for got, key in ((loss, "loss"), (gs, "grad_log_logit_scale"), (gb, "grad_logit_bias")):
        want = float(z[f"{tag}/{key}"])
        assert abs(float(got) - want) <= 1e-5 * abs(want) + 1e-7, (key, float(got), want)
    for got, key in ((gi, "grad_image"), (gt, "grad_text")):
        want = _t(z[f"{tag}/{key}"]).to(DEV)
        err = float((got - want).abs().max())
        assert err <= 1e-5 * float(want.abs().max()), (key, err)


def test_large_vs_float64():
    g = torch.Generator(device=DEV).manual_seed(3)
    n, e = 4096, 512
    fi0 = torch.nn.functional.normalize(torch.randn(n, e, device=DEV, generator=g), dim=-1)
    ft0 = torch.nn.functional.normalize(fi0 + 0.7 * torch.randn(n, e, device=DEV, generator=g), dim=-1)
    fi, ft, ls, lb = _leaves(fi0.cpu(), ft0.cpu(), math.log(10.0) + 0.5, -6.0)
    loss, gi, gt, gs, gb = _step(fi, ft, ls, lb)
    want = _f64(fi0, ft0, math.exp(math.log(10.0) + 0.5), -6.0, 0)
    assert abs(float(loss) - float(want[0])) <= 1e-4 * abs(float(want[0]))
    for got, w in ((gi, want[1]), (gt, want[2])):
        assert float((got.double() - w).abs().max()) <= 1e-4 * float(w.abs().max())
    assert abs(float(gs) - float(want[3])) <= 1e-4 * abs(float(want[3]))
    assert abs(float(gb) - float(want[4])) <= 1e-4 * abs(float(want[4]))
    # two runs: bit-identical loss and gradients (no float atomics; partials summed in a fixed order)
    fi2, ft2, ls2, lb2 = _leaves(fi0.cpu(), ft0.cpu(), math.log(10.0) + 0.5, -6.0)
    again = _step(fi2, ft2, ls2, lb2)
    for a, b in zip((loss, gi, gt, gs, gb), again):
        assert torch.equal(a, b)


@pytest.mark.parametrize("e", list(ops.FUSED_CE_DIMS) + [48])      # every fused walk instantiation, and the dense path
@pytest.mark.parametrize("c_mult,pos_off", [(1, -1), (3, 2 * 70), (3, 70)])
def test_negative_only_and_nonsquare_blocks(e, c_mult, pos_off):
    g = torch.Generator(device=DEV).manual_seed(5)
    b = 70
    fi0 = torch.nn.functional.normalize(torch.randn(b, e, device=DEV, generator=g), dim=-1)
    ft0 = torch.nn.functional.normalize(torch.randn(c_mult * b, e, device=DEV, generator=g), dim=-1)
    fi, ft, ls, lb = _leaves(fi0.cpu(), ft0.cpu(), math.log(10.0), -10.0)
    loss, gi, gt, gs, gb = _step(fi, ft, ls, lb, pos_off)
    want = _f64(fi0, ft0, 10.0, -10.0, pos_off)
    assert abs(float(loss) - float(want[0])) <= 1e-5 * abs(float(want[0]))
    for got, w in ((gi, want[1]), (gt, want[2])):
        assert float((got.double() - w).abs().max()) <= 1e-5 * float(w.abs().max())
    assert abs(float(gs) - float(want[3])) <= 1e-5 * abs(float(want[3])) + 1e-7
    assert abs(float(gb) - float(want[4])) <= 1e-5 * abs(float(want[4])) + 1e-7


@pytest.mark.parametrize("e", [512, 48])
def test_no_grad_forward(e):
    g = torch.Generator(device=DEV).manual_seed(9)
    fi = torch.nn.functional.normalize(torch.randn(300, e, device=DEV, generator=g), dim=-1)
    ft = torch.nn.functional.normalize(torch.randn(300, e, device=DEV, generator=g), dim=-1)
    scale, bias = torch.tensor(10.0, device=DEV), torch.tensor(-10.0, device=DEV)
    with torch.no_grad():
        got = SigLipLoss()(fi, ft, scale, bias)
    assert not got.requires_grad
    want = _f64(fi, ft, 10.0, -10.0, 0)[0]
    assert abs(float(got) - float(want)) <= 1e-5 * abs(float(want))
    d = SigLipLoss()(fi, ft, scale, bias, output_dict=True)
    assert set(d) == {"contrastive_loss"} and float(d["contrastive_loss"]) == float(got)


def _grad_sample_index(numel, n):
    """make_golden.grad_sample_index: evenly strided element indices of a flattened gradient"""
    if numel <= n:
        return torch.arange(numel)
    return (torch.arange(n, dtype=torch.int64) * numel) // n


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_clip_model_vs_reference_fixture(golden_dir, precision):
    """siglip_tiny.npz: the tiny model of tiny_clip.npz with logit_bias = -10 through the reference's towers and SigLipLoss.
    Weights and batch are regenerated from their seeds (checksummed against the fixture)."""
    from oracle import clip_oracle as O
    z = _load(golden_dir, "siglip_tiny.npz")
    cfg = O.TINY
    sd = O.perturb_state_dict(O.init_state_dict(cfg, seed=0), seed=1)
    sd["logit_bias"] = torch.tensor(-10.0)
    image, text = O.synthetic_batch(cfg, 8, seed=1234)
    chk = np.array([float(sd[k].double().sum()) for k in sorted(sd.keys())])
    assert np.allclose(chk, z["sd_checksum"], rtol=1e-9, atol=1e-9)
    assert np.allclose([float(image.double().sum()), float(text.double().sum())], z["batch_checksum"], rtol=1e-9, atol=1e-9)
    model, _, _ = create_model_and_transforms("ViT-tiny-test", precision=precision, device=DEV, output_dict=True,
                                              init_logit_bias=-10.0)
    model.load_state_dict({k: v.clone() for k, v in sd.items()}, strict=True)
    model.train()
    image = image.to(DEV)
    out = model(image.bfloat16() if precision == "bf16" else image, text.to(DEV))
    assert "logit_bias" in out
    loss = SigLipLoss()(**out)
    loss.backward()
    loss = float(loss.detach())
    grads = {k: p.grad.detach().float().cpu() for k, p in model.named_parameters()}
    names = [str(n) for n in z["grad_names"]]
    assert sorted(names) == sorted(grads)
    fi, ft = out["image_features"].detach().float().cpu(), out["text_features"].detach().float().cpu()
    if precision == "fp32":
        assert float((fi - _t(z["image_features"])).abs().max()) < 1e-5
        assert float((ft - _t(z["text_features"])).abs().max()) < 1e-5
        assert abs(loss - float(z["loss"])) < 1e-5 * abs(float(z["loss"]))
        n_s = z["grad_sample"].shape[1]
        for i, k in enumerate(names):
            g = grads[k].reshape(-1)
            got = g[_grad_sample_index(g.numel(), n_s)]
            want = _t(z["grad_sample"][i][:got.numel()]).float()
            scale = float(z["grad_maxabs"][i]) + 1e-8
            assert float((got - want).abs().max()) < 2e-3 * scale, k
            assert abs(float(g.double().norm()) - float(z["grad_norms"][i])) < 2e-3 * float(z["grad_norms"][i]) + 1e-8, k
    else:       # the bars of tests/test_colxlip_gpu.py: feature cosines > 0.999, loss within 2e-2, gradient norms within 3 %
        for got, key in ((fi, "image_features"), (ft, "text_features")):
            assert float((got * _t(z[key])).sum(-1).min()) > 0.999, key
        assert abs(loss - float(z["loss"])) < 2e-2
        gmax = float(np.max(z["grad_norms"]))
        for i, k in enumerate(names):
            want = float(z["grad_norms"][i])
            got = float(grads[k].double().norm())
            if k != "logit_scale" and want > 1e-7:
                assert max(0.0, abs(got - want) - 3e-5 * gmax) / want < 0.03, (k, got, want)


def test_main_trains_with_siglip(tmp_path, caplog):
    from colxlip_amd.main import main
    steps = 4
    argv = ["--model", "ViT-small-test", "--dataset-type", "synthetic", "--precision", "fp32", "--batch-size", "8", "--siglip",
            "--lr", "1e-3", "--wd", "0.1", "--lr-scheduler", "const", "--warmup", "1", "--epochs", "1",
            "--train-num-samples", str(8 * steps), "--logs-dir", str(tmp_path), "--name", "sig", "--log-every-n-steps", "1",
            "--seed", "3", "--save-frequency", "1"]
    with caplog.at_level(logging.INFO):
        assert main(argv) == 0
    lines = [r.getMessage() for r in caplog.records if r.getMessage().startswith("Train Epoch")]
    assert len(lines) == steps and all("Contrastive_loss" in l for l in lines)
    vals = [float(l.split("Contrastive_loss: ")[1].split()[0]) for l in lines]
    assert all(math.isfinite(v) and v > 0 for v in vals)
    ck = torch.load(os.path.join(tmp_path, "sig", "checkpoints", "epoch_1.pt"), map_location="cpu", weights_only=True)
    sd = ck["state_dict"]
    sd = {k[len("module."):] if k.startswith("module.") else k: v for k, v in sd.items()}
    assert abs(float(sd["logit_scale"]) - math.log(10)) < 0.1
    assert float(sd["logit_bias"]) != -10.0 and math.isfinite(float(sd["logit_bias"]))
