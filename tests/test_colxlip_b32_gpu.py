"""ViT-B-32-colxlip -- the architecture of the reference's ColXLIP launch line (src/colxlip.sh:38, alpha 0.7; 49 image tokens) --
stepped once at batch 8 against tests/golden/colxlip_b32_batch8.npz, which tests/golden/make_golden_colxlip_b32.py wrote by
executing the reference's own `ColXLIP.encode_image / encode_text / forward` and ColClipLoss.

The checks and bounds are those of tests/test_colxlip_gpu.py::test_colxlip_step_vs_reference_fixture.  In bf16 the token loss
runs on the fused MaxSim for fewer than 64 tokens per image (csrc/gemm_nt_maxsim.h); the same step with CLIPX_MAXSIM_FUSED=0
(the similarity matrix written and reduced by a second kernel) is run next to it and both routes' errors are printed."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import clip_oracle as O  # noqa: E402  (checker only)
from colxlip_amd import ops  # noqa: E402
from colxlip_amd.loss import ColClipLoss  # noqa: E402
from tests.test_colxlip_gpu import _model  # noqa: E402
from tests.test_configs_gpu import _direction, _load, _record, _t  # noqa: E402

DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODEL = "ViT-B-32-colxlip"


@pytest.fixture(scope="module")
def case(golden_dir):
    z = _load(golden_dir, "colxlip_b32_batch8.npz")
    with open(os.path.join(ROOT, "colxlip_amd", "model_configs", MODEL + ".json")) as f:
        cfg = O.ClipCfg.from_model_json(json.load(f))
    sd = O.colxlip_state_dict(cfg)
    chk = np.array([float(sd[k].double().sum()) for k in sorted(sd.keys())])
    assert np.allclose(chk, z["sd_checksum"], rtol=1e-9, atol=1e-9), "RNG did not reproduce the fixture's weights"
    image, text = O.synthetic_batch(cfg, int(z["batch"]), seed=int(z["data_seed"]))
    assert np.array_equal(text.numpy(), z["text"])
    return z, sd, image, text


def _step(case, precision):
    """one forward + ColClipLoss + backward -> the figures test_colxlip_step_vs_reference_fixture looks at"""
    z, sd, image, text = case
    alpha = float(z["alpha"])
    model = _model(MODEL, sd, precision)
    assert type(model).__name__ == "ColXLIP"
    assert sorted(k for k, _ in model.named_parameters()) == sorted(str(n) for n in z["grad_names"])
    model.zero_grad(set_to_none=True)
    x = image.to(DEV).bfloat16() if precision == "bf16" else image.to(DEV)
    out = model(x, text.to(DEV))
    assert set(out) == {"image_features", "text_features", "token_image_features", "token_text_features", "logit_scale"}
    assert out["token_image_features"].shape == (8, 49, 512)
    res = ColClipLoss(alpha=alpha)(**out, output_dict=True)
    res["total_loss"].backward()
    torch.cuda.synchronize()
    grads = {k: p.grad.detach().float() for k, p in model.named_parameters()}
    o = {k: v.detach().float().cpu() for k, v in out.items()}
    f = {"feat_err": {}, "feat_cos": {}}
    for k in ("image_features", "text_features", "token_image_features", "token_text_features"):
        got, want = (o[k], _t(z[k])) if k in z else (o[k][:, ::4], _t(z[k + "_s4"]))
        assert got.shape == want.shape, k
        f["feat_err"][k] = float((got - want).abs().max())
        f["feat_cos"][k] = float((got * want).sum(-1).min())
    eot = text.argmax(-1)
    tt = o["token_text_features"]
    for s in range(text.shape[0]):
        assert float((tt[s, int(eot[s]):] - tt[s, -1]).abs().max()) == 0.0
    f["loss_err"] = {n: abs(float(res[key].detach()) - float(z[n])) for n, key in (("global_loss", "global_contrastive_loss"),
                                                                          ("token_loss", "token_contrastive_loss"), ("total_loss", "total_loss"))}
    ltt = ColClipLoss(alpha=alpha).get_logits(out["image_features"], out["text_features"], out["token_image_features"],
                                              out["token_text_features"], out["logit_scale"])["logits_per_text_token"]
    f["logit_err"] = float((ltt.detach().float().cpu() - _t(z["logits_per_text_token"])).abs().max())
    gmax = float(np.max(z["grad_norms"]))
    floor = 0.0 if precision == "fp32" else 3e-5 * gmax
    worst, worst_name = 0.0, ""
    for name, norm in zip(z["grad_names"], z["grad_norms"]):
        g = float(grads[str(name)].double().norm())
        rel = max(0.0, abs(g - norm) - floor) / (norm + 1e-12)
        if str(name) != "logit_scale" and norm > 1e-7 and rel > worst:
            worst, worst_name = rel, str(name)
    f["worst"], f["worst_name"] = worst, worst_name
    i_ls = [str(n) for n in z["grad_names"]].index("logit_scale")
    f["err_ls"] = abs(float(grads["logit_scale"]) - float(z["grad_sample"][i_ls][0]))
    f["d_el"], f["d_el_name"], f["d_cos"], f["d_cos_name"], f["d_mean"] = _direction(z, grads, precision, max(floor, 1e-7 * gmax))
    return f


def _line(tag, precision, f):
    return (f"ColXLIP {MODEL} b8 {precision} [{tag}]: feature err " + " ".join(f"{v:.2e}" for v in f["feat_err"].values())
            + " min cos " + " ".join(f"{v:.6f}" for v in f["feat_cos"].values())
            + f"; loss err global {f['loss_err']['global_loss']:.2e} token {f['loss_err']['token_loss']:.2e} total {f['loss_err']['total_loss']:.2e}"
            f"; max|token logit err| {f['logit_err']:.2e}; worst grad-norm rel err {f['worst']:.3e} ({f['worst_name']})"
            f"; |d logit_scale| err {f['err_ls']:.2e}; worst element err {f['d_el']:.2e} ({f['d_el_name']})"
            f"; sketch cosine worst {f['d_cos']:.5f} ({f['d_cos_name']}) mean {f['d_mean']:.5f}")


def test_b32_step_fp32(case):
    """fp32 (the exact-fp32 kernels; measured: losses within 5e-7, worst gradient-norm error 1.4e-6)"""
    f = _step(case, "fp32")
    line = _line("fp32 route", "fp32", f)
    print(line)
    _record(line)
    assert max(f["feat_err"].values()) < 1e-4, f["feat_err"]
    assert max(f["loss_err"].values()) < 1e-3 and f["logit_err"] < 1e-3
    assert max(f["loss_err"].values()) < 2e-5, f["loss_err"]
    assert f["worst"] < 5e-3, (f["worst_name"], f["worst"])
    assert f["d_el"] < 1e-3, (f["d_el_name"], f["d_el"])
    assert f["err_ls"] < 1e-4


def test_b32_step_bf16_fused_and_unfused(case, monkeypatch):
    """The bf16 step on the fused MaxSim, held to the B/16 test's bf16 bounds; the unfused route's figures are printed beside it.
    Measured on an MI355X, fused / unfused: token loss error 1.71e-3 / 1.84e-3, token logit error 1.14e-2 / 1.08e-2, worst
    gradient-norm error 1.0e-2 (text_token_layer.1.weight) / 2.4e-3, worst sketch cosine 0.9974 / 0.9985 -- every bound held by both."""
    gemms = []
    gemm = ops.maxsim_gemm
    monkeypatch.setattr(ops, "maxsim_gemm", lambda *args: (gemms.append(args[2:4]), gemm(*args))[1])
    f = _step(case, "bf16")
    assert (8, 49) in gemms                                     # the token loss ran on the fused MaxSim
    line = _line("fused MaxSim", "bf16", f)
    print(line)
    _record(line)
    del gemms[:]
    monkeypatch.setenv("CLIPX_MAXSIM_FUSED", "0")
    u = _step(case, "bf16")
    assert not gemms
    print(_line("CLIPX_MAXSIM_FUSED=0", "bf16", u))
    assert min(f["feat_cos"]["image_features"], f["feat_cos"]["text_features"]) > 0.999, f["feat_cos"]
    assert min(f["feat_cos"]["token_image_features"], f["feat_cos"]["token_text_features"]) > 0.995, f["feat_cos"]
    assert max(f["loss_err"].values()) < 2e-2, f["loss_err"]
    assert f["worst"] < 0.03, (f["worst_name"], f["worst"])
    assert f["err_ls"] < 3e-3
    assert f["d_mean"] > 0.99, f["d_mean"]
    assert f["d_cos"] > 0.97, (f["d_cos_name"], f["d_cos"])
