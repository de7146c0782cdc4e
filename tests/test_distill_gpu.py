"""DistillClipLoss on the MI355X (csrc/loss_distill.hip): the fused and materialising kernels against the reference's own
DistillClipLoss (tests/golden/distill_loss.npz, written by make_golden_distill.py), a float64 evaluation at N = 4096,
non-square local blocks, the no_grad forward, run-to-run bit identity, a student + teacher model pair (distill_tiny.npz)
and `main --distill-model ... --distill-pretrained ...`."""
import logging
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from colxlip_amd import DistillClipLoss, create_model_and_transforms, ops
from colxlip_amd.loss import distill_ce

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# make_golden_distill.W1_CASES: (tag, b, Es, Et, teacher needs grad)
CASES = (("a", 16, 64, 64, False), ("b", 100, 512, 768, False), ("c", 70, 48, 96, False), ("d", 40, 64, 64, False),
         ("e", 24, 64, 128, True))


def _load(golden_dir, name):
    z = np.load(os.path.join(golden_dir, name), allow_pickle=False)
    return {k: z[k] for k in z.files}


def _t(a):
    return torch.from_numpy(np.asarray(a))


def _case_inputs(i, tag, b, es, et):
    """make_golden_distill.case_inputs"""
    g = torch.Generator().manual_seed(21 + i)
    fi = F.normalize(torch.randn(b, es, generator=g), dim=-1)
    ft = F.normalize(torch.randn(b, es, generator=g), dim=-1)
    tfi = F.normalize(torch.randn(b, et, generator=g), dim=-1)
    tft = F.normalize(torch.randn(b, et, generator=g), dim=-1)
    if tag == "d":
        tft = F.normalize(tfi + 0.05 * tft, dim=-1)
    return fi, ft, tfi, tft


def _f64(fi, ft, s, tfi, tft, ts, off=0, symmetric=True):
    """both losses of one problem in float64 on the device: rows of s = s*fi @ ft.T against t, w = 0.5 / rows"""
    S = s * fi.double() @ ft.double().T
    T = ts * tfi.double() @ tft.double().T
    r = S.shape[0]
    lab = torch.arange(r, device=S.device) + off

    def d(tl, sl):
        return -(tl.softmax(1) * sl.log_softmax(1)).sum(1).sum() * 0.5 / r

    c = F.cross_entropy(S, lab, reduction="sum") * 0.5 / r
    di = d(T, S)
    if symmetric:
        c = c + F.cross_entropy(S.T, lab, reduction="sum") * 0.5 / r
        di = di + d(T.T, S.T)
    return c, di


@pytest.mark.parametrize("i", range(len(CASES)))
def test_kernels_vs_reference_fixture(golden_dir, i):
    """a, d: fused Es = Et = 64 (d: teacher softmax saturated); b: fused (512, 768), b = 100; c: (48, 96), the materialising
    path; e: the teacher features and scale need a gradient (materialising path with dt)"""
    z = _load(golden_dir, "distill_loss.npz")
    tag, b, es, et, tgrad = CASES[i]
    p = f"{tag}/"
    if p + "image_features" in z:
        fi, ft, tfi, tft = (_t(z[p + k]) for k in ("image_features", "text_features", "dist_image_features",
                                                     "dist_text_features"))
    else:
        fi, ft, tfi, tft = _case_inputs(i, tag, b, es, et)
        assert np.allclose([float(v.double().sum()) for v in (fi, ft, tfi, tft)], z[p + "input_checksum"], rtol=1e-9, atol=1e-9)
    fi, ft, tfi, tft = (x.to(DEV).float() for x in (fi, ft, tfi, tft))
    fi.requires_grad_(True)
    ft.requires_grad_(True)
    if tgrad:
        tfi.requires_grad_(True)
        tft.requires_grad_(True)
    ls = _t(z[p + "log_logit_scale"]).to(DEV).float().reshape(()).requires_grad_(True)
    tls = _t(z[p + "dist_log_logit_scale"]).to(DEV).float().reshape(()).requires_grad_(tgrad)
    c, d = DistillClipLoss()(fi, ft, ls.exp(), tfi, tft, tls.exp())
    (c + float(z["dist_w"]) * d).backward()
    checks = [(c, "contrastive_loss"), (d, "distill_loss"), (ls.grad, "grad_log_logit_scale")]
    grads = [(fi.grad, "grad_image"), (ft.grad, "grad_text")]
    if tgrad:
        checks.append((tls.grad, "grad_dist_log_logit_scale"))
        grads += [(tfi.grad, "grad_dist_image"), (tft.grad, "grad_dist_text")]
    for got, key in checks:
        want, got = float(z[p + key]), float(got.detach())
        assert abs(got - want) <= 1e-5 * abs(want) + 1e-7, (key, got, want)
    for got, key in grads:
        want = _t(z[p + key]).to(DEV)
        err = float((got - want).abs().max())
        assert err <= 1e-5 * float(want.abs().max()), (key, err)


def _problem(n, es, et, seed, dev=DEV):
    g = torch.Generator(device=dev).manual_seed(seed)
    fi = F.normalize(torch.randn(n, es, device=dev, generator=g), dim=-1)
    ft = F.normalize(fi[:, :es] + 0.8 * torch.randn(n, es, device=dev, generator=g), dim=-1)
    tfi = F.normalize(torch.randn(n, et, device=dev, generator=g), dim=-1)
    tft = F.normalize(tfi + 0.5 * torch.randn(n, et, device=dev, generator=g), dim=-1)
    return fi, ft, tfi, tft


def _run(fi0, ft0, tfi, tft, log_s, log_ts, gd_w=0.75, off=0, symmetric=True):
    fi = fi0.clone().requires_grad_(True)
    ft = ft0.clone().requires_grad_(True)
    ls = torch.tensor(log_s, device=DEV).requires_grad_(True)
    c, d = distill_ce(fi, ft, ls.exp(), tfi, tft, torch.tensor(math.exp(log_ts), device=DEV), off, symmetric)
    (c + gd_w * d).backward()
    return c.detach(), d.detach(), fi.grad, ft.grad, ls.grad


def _f64_grads(fi, ft, log_s, tfi, tft, log_ts, gd_w=0.75, off=0, symmetric=True):
    fi = fi.double().requires_grad_(True)
    ft = ft.double().requires_grad_(True)
    ls = torch.tensor(log_s, device=DEV, dtype=torch.float64).requires_grad_(True)
    c, d = _f64(fi, ft, ls.exp(), tfi, tft, math.exp(log_ts), off, symmetric)
    (c + gd_w * d).backward()
    return c.detach(), d.detach(), fi.grad, ft.grad, ls.grad


def test_large_vs_float64_and_bit_identical():
    n = 4096
    fi, ft, tfi, tft = _problem(n, 512, 768, 3)
    got = _run(fi, ft, tfi, tft, math.log(20.0), math.log(50.0))
    want = _f64_grads(fi, ft, math.log(20.0), tfi, tft, math.log(50.0))
    for a, w in zip(got[:2], want[:2]):
        assert abs(float(a) - float(w)) <= 1e-4 * abs(float(w))
    for a, w in zip(got[2:4], want[2:4]):
        assert float((a.double() - w).abs().max()) <= 1e-4 * float(w.abs().max())
    assert abs(float(got[4]) - float(want[4])) <= 1e-4 * abs(float(want[4])) + 1e-6
    again = _run(fi, ft, tfi, tft, math.log(20.0), math.log(50.0))      # no float atomics: the same bits every run
    for a, b in zip(got, again):
        assert torch.equal(a, b)


# every fused dim on the student side (the walk's instantiations) and on the teacher side; (48, 96) takes the dense path
@pytest.mark.parametrize("es,et", [(64, 128), (16, 1024), (32, 768), (128, 640), (256, 512), (512, 256), (640, 32), (768, 16),
                                   (1024, 64), (48, 96)])
@pytest.mark.parametrize("c_mult,off", [(3, 70), (3, 140), (2, 0)])
def test_nonsquare_local_blocks(es, et, c_mult, off):
    """the local-loss problem: b rows against W*b columns, labels at column r + b*rank"""
    b = 70
    g = torch.Generator(device=DEV).manual_seed(5)
    fi = F.normalize(torch.randn(b, es, device=DEV, generator=g), dim=-1)
    ft = F.normalize(torch.randn(c_mult * b, es, device=DEV, generator=g), dim=-1)
    tfi = F.normalize(torch.randn(b, et, device=DEV, generator=g), dim=-1)
    tft = F.normalize(torch.randn(c_mult * b, et, device=DEV, generator=g), dim=-1)
    got = _run(fi, ft, tfi, tft, math.log(10.0), math.log(40.0), off=off, symmetric=False)
    want = _f64_grads(fi, ft, math.log(10.0), tfi, tft, math.log(40.0), off=off, symmetric=False)
    for a, w in zip(got[:2], want[:2]):
        assert abs(float(a) - float(w)) <= 1e-5 * abs(float(w))
    for a, w in zip(got[2:4], want[2:4]):
        assert float((a.double() - w).abs().max()) <= 1e-5 * float(w.abs().max())
    assert abs(float(got[4]) - float(want[4])) <= 1e-5 * abs(float(want[4])) + 1e-7


@pytest.mark.parametrize("es,et", [(512, 768), (48, 96)])
def test_no_grad_forward(es, et):
    fi, ft, tfi, tft = _problem(300, es, et, 9)
    scale, tscale = torch.tensor(10.0, device=DEV), torch.tensor(30.0, device=DEV)
    with torch.no_grad():
        c, d = DistillClipLoss()(fi, ft, scale, tfi, tft, tscale)
    assert not c.requires_grad and not d.requires_grad
    wc, wd = _f64(fi, ft, 10.0, tfi, tft, 30.0)
    assert abs(float(c) - float(wc)) <= 1e-5 * abs(float(wc))
    assert abs(float(d) - float(wd)) <= 1e-5 * abs(float(wd))
    out = DistillClipLoss()(fi.requires_grad_(True), ft, scale, tfi, tft, tscale, output_dict=True)
    assert set(out) == {"contrastive_loss", "distill_loss"}
    assert float(out["contrastive_loss"]) == float(c) and float(out["distill_loss"]) == float(d)


def _grad_sample_index(numel, n):
    """make_golden.grad_sample_index: evenly strided element indices of a flattened gradient"""
    if numel <= n:
        return torch.arange(numel)
    return (torch.arange(n, dtype=torch.int64) * numel) // n


def _tiny_weights():
    from oracle import clip_oracle as O
    small = O.ClipCfg(embed_dim=64, image_size=64, patch_size=16, vision_width=128, vision_layers=2, context_length=77,
                      vocab_size=1024, text_width=128, text_heads=2, text_layers=2)
    teacher = O.ClipCfg(embed_dim=128, image_size=64, patch_size=16, vision_width=192, vision_layers=2, context_length=77,
                        vocab_size=1024, text_width=192, text_heads=3, text_layers=2)
    sd = O.perturb_state_dict(O.init_state_dict(small, seed=0), seed=1)
    tsd = O.perturb_state_dict(O.init_state_dict(teacher, seed=2), seed=3)
    image, text = O.synthetic_batch(small, 8, seed=1234)
    return sd, tsd, image, text


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_student_teacher_vs_reference_fixture(golden_dir, precision):
    """distill_tiny.npz: ViT-small-test student, ViT-teacher-test teacher, the reference's towers and DistillClipLoss"""
    z = _load(golden_dir, "distill_tiny.npz")
    sd, tsd, image, text = _tiny_weights()
    assert np.allclose([float(sd[k].double().sum()) for k in sorted(sd)], z["sd_checksum"], rtol=1e-9, atol=1e-9)
    assert np.allclose([float(tsd[k].double().sum()) for k in sorted(tsd)], z["teacher_checksum"], rtol=1e-9, atol=1e-9)
    assert np.allclose([float(image.double().sum()), float(text.double().sum())], z["batch_checksum"], rtol=1e-9, atol=1e-9)
    model, _, _ = create_model_and_transforms("ViT-small-test", precision=precision, device=DEV, output_dict=True)
    model.load_state_dict({k: v.clone() for k, v in sd.items()}, strict=True)
    model.train()
    teacher, _, _ = create_model_and_transforms("ViT-teacher-test", precision=precision, device=DEV, output_dict=True)
    teacher.load_state_dict({k: v.clone() for k, v in tsd.items()}, strict=True)
    teacher.eval()
    image = image.to(DEV)
    image = image.bfloat16() if precision == "bf16" else image
    text = text.to(DEV)
    with torch.no_grad():
        tout = teacher(image, text)
    out = model(image, text)
    out.update({f"dist_{k}": v for k, v in tout.items()})
    losses = DistillClipLoss()(**out, output_dict=True)
    (losses["contrastive_loss"] + losses["distill_loss"]).backward()
    c, d = float(losses["contrastive_loss"]), float(losses["distill_loss"])
    grads = {k: p.grad.detach().float().cpu() for k, p in model.named_parameters()}
    assert all(p.grad is None for p in teacher.parameters())
    names = [str(n) for n in z["grad_names"]]
    assert sorted(names) == sorted(grads)
    feats = {k: out[k].detach().float().cpu() for k in ("image_features", "text_features", "dist_image_features",
                                                         "dist_text_features")}
    if precision == "fp32":
        for k, v in feats.items():
            assert float((v - _t(z[k])).abs().max()) < 1e-5, k
        assert abs(c - float(z["contrastive_loss"])) < 1e-5 * abs(float(z["contrastive_loss"]))
        assert abs(d - float(z["distill_loss"])) < 1e-5 * abs(float(z["distill_loss"]))
        n_s = z["grad_sample"].shape[1]
        for i, k in enumerate(names):
            g = grads[k].reshape(-1)
            got = g[_grad_sample_index(g.numel(), n_s)]
            want = _t(z["grad_sample"][i][:got.numel()]).float()
            scale = float(z["grad_maxabs"][i]) + 1e-8
            assert float((got - want).abs().max()) < 2e-3 * scale, k
            assert abs(float(g.double().norm()) - float(z["grad_norms"][i])) < 2e-3 * float(z["grad_norms"][i]) + 1e-8, k
    else:       # the bars of tests/test_siglip_gpu.py: feature cosines > 0.999, losses within 2e-2, gradient norms within 3 %
        for k, v in feats.items():
            assert float((v * _t(z[k])).sum(-1).min()) > 0.999, k
        assert abs(c - float(z["contrastive_loss"])) < 2e-2
        assert abs(d - float(z["distill_loss"])) < 2e-2
        gmax = float(np.max(z["grad_norms"]))
        for i, k in enumerate(names):
            want = float(z["grad_norms"][i])
            got = float(grads[k].double().norm())
            if k != "logit_scale" and want > 1e-7:
                assert max(0.0, abs(got - want) - 3e-5 * gmax) / want < 0.03, (k, got, want)


def _argv(tmp_path, name, steps, teacher_ckpt=None):
    argv = ["--model", "ViT-small-test", "--dataset-type", "synthetic", "--precision", "fp32", "--batch-size", "8",
            "--lr", "1e-3", "--wd", "0.1", "--lr-scheduler", "const", "--warmup", "1", "--epochs", "1",
            "--train-num-samples", str(8 * steps), "--logs-dir", str(tmp_path), "--name", name, "--log-every-n-steps", "1",
            "--seed", "3", "--save-frequency", "1"]
    if teacher_ckpt:
        argv += ["--distill-model", "ViT-teacher-test", "--distill-pretrained", teacher_ckpt]
    return argv


def test_main_trains_with_a_teacher(tmp_path, caplog, monkeypatch):
    from colxlip_amd import main as main_mod
    from colxlip_amd import train as train_mod
    _, tsd, _, _ = _tiny_weights()
    ckpt = str(tmp_path / "teacher.pt")
    torch.save(tsd, ckpt)
    first = {}
    teachers = []
    orig_single = train_mod._StepRunner._single

    def spy(self, images, texts):
        if not first:
            first.update(images=images.clone(), texts=texts.clone(),
                         sd={k: v.detach().clone() for k, v in train_mod.unwrap_model(self.model).state_dict().items()})
            teachers.append(self.dist_model)
        return orig_single(self, images, texts)

    monkeypatch.setattr(train_mod._StepRunner, "_single", spy)
    steps = 4
    with caplog.at_level(logging.INFO):
        assert main_mod.main(_argv(tmp_path, "dist", steps, ckpt)) == 0
    lines = [r.getMessage() for r in caplog.records if r.getMessage().startswith("Train Epoch")]
    assert len(lines) == steps and all("Contrastive_loss" in l and "Distill_loss" in l for l in lines)
    c0 = float(lines[0].split("Contrastive_loss: ")[1].split()[0])
    d0 = float(lines[0].split("Distill_loss: ")[1].split()[0])
    assert all(math.isfinite(float(l.split("Distill_loss: ")[1].split()[0])) for l in lines)
    # the teacher: bit-unchanged weights, eval mode, never given a gradient
    teacher = teachers[0]
    assert teacher is not None and not teacher.training
    tsd_after = teacher.state_dict()
    assert all(torch.equal(tsd_after[k].cpu(), tsd[k]) for k in tsd)
    assert all(p.grad is None for p in teacher.parameters())
    # the first step's losses, recomputed from its batch and the student's starting weights
    student, _, _ = create_model_and_transforms("ViT-small-test", precision="fp32", device=DEV, output_dict=True)
    student.load_state_dict(first["sd"])
    student.train()
    with torch.no_grad():
        tout = teacher(first["images"], first["texts"])
        out = student(first["images"], first["texts"])
    out.update({f"dist_{k}": v for k, v in tout.items()})
    want = DistillClipLoss()(**out, output_dict=True)
    assert abs(c0 - float(want["contrastive_loss"])) <= 1e-4 * abs(float(want["contrastive_loss"]))
    assert abs(d0 - float(want["distill_loss"])) <= 1e-4 * abs(float(want["distill_loss"]))
    # the student checkpoint holds exactly what a run without a teacher holds
    monkeypatch.setattr(train_mod._StepRunner, "_single", orig_single)
    assert main_mod.main(_argv(tmp_path, "plain", 1)) == 0
    ck = torch.load(os.path.join(tmp_path, "dist", "checkpoints", "epoch_1.pt"), map_location="cpu", weights_only=True)
    ck0 = torch.load(os.path.join(tmp_path, "plain", "checkpoints", "epoch_1.pt"), map_location="cpu", weights_only=True)
    assert set(ck) == set(ck0)
    assert set(ck["state_dict"]) == set(ck0["state_dict"])
    assert len(ck["optimizer"]["state"]) == len(ck0["optimizer"]["state"])
