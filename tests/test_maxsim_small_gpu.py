"""The fused MaxSim for 16 <= q < 64 image tokens per image (ViT-B-32-colxlip has 49): the per-image epilogue of the ping-pong NT
GEMM (csrc/gemm_nt_maxsim.h, `nt_maxsim_seg_epilogue`), the fold kernels of csrc/colbert.hip on its [2 * image + half] partials,
and both routes that use them: ColClipLoss (`_MaxSimFused`) and the forward-only scorer (`ops.maxsim_scores`).

Pinning: the reference's arithmetic (loss.py:20-46) in fp32 on the same bf16 values, with the bounds of
tests/test_model_gpu.py::test_maxsim_fused_vs_torch and tests/test_late_interaction_gpu.py; a model with 49 image tokens against
the CPU oracle."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from colxlip_amd import ops  # noqa: E402
from colxlip_amd import loss as LS  # noqa: E402
from oracle import clip_oracle as O  # noqa: E402
from tests import late_interaction_ref as R  # noqa: E402
from tests.late_interaction_ref import Q49, Q49_MODEL  # noqa: E402

DEV = "cuda"

# (ni, q, nt, n, e)
SMALL_SHAPES = [
    (8, 49, 8, 77, 512),        # ViT-B/32: up to 3 images per 64-column slot, 2 tile columns
    (8, 63, 3, 20, 128),        # 2 images per slot, like the q >= 64 form
    (5, 32, 6, 9, 128),         # slots and images aligned; N = 160 < one tile
    (8, 33, 4, 7, 256),
    (3, 24, 5, 11, 128),        # up to 4 images per slot, N = 72
    (40, 31, 4, 7, 128),        # 5 tile columns, the last one partial
    (8, 17, 6, 9, 128),         # up to 5 images per slot
    (16, 16, 4, 7, 128),
]


@pytest.mark.parametrize("ni,q,nt,n,e", SMALL_SHAPES)
def test_maxsim_small_vs_torch(ni, q, nt, n, e, monkeypatch):
    """tests/test_model_gpu.py::test_maxsim_fused_vs_torch for fewer than 64 tokens per image, with its bounds: forward 2e-5,
    gradients 6e-3 in relative norm and cosine > 0.9999 against the fp32 einsum on the same bf16 values; 2e-2 against the
    unfused route where that one takes the shape.  Text shaped like ColXLIP's output: one vector at / behind a per-sample EOT,
    sample 1 exact zeros there, sample 2 without duplicates."""
    g = torch.Generator().manual_seed(100 + q)
    ti = torch.nn.functional.normalize(torch.randn(ni, q, e, generator=g), dim=-1)
    tt = torch.nn.functional.normalize(torch.randn(nt, n, e, generator=g), dim=-1)
    tail = torch.nn.functional.normalize(torch.randn(e, generator=g), dim=-1)
    for m in range(nt):
        eot = 2 + (5 * m) % (n - 2)
        if m == 1:
            tt[m, eot:] = 0.0
        elif m != 2:
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
    ref = mx.sum(-1) / ((mx != 0).float().sum(-1) + 1e-8)
    ref.backward(gout)
    err = float((out - ref).detach().abs().max())
    print(f"maxsim small ({ni},{q},{nt},{n},{e}): forward err {err:.3e}")
    assert err < 2e-5, err
    for got, want, name in ((a.grad.float(), a32.grad, "image tokens"), (b.grad.float(), b32.grad, "text tokens")):
        rel = float((got - want).norm() / want.norm())
        cos = float((got * want).sum() / (got.norm() * want.norm()))
        print(f"  {name}: gradient rel err {rel:.3e} cosine {cos:.6f}")
        assert rel < 6e-3, (name, rel)
        assert cos > 0.9999, (name, cos)
    assert torch.equal(b.grad[0, 2], b.grad[0, n - 1]) and float(b.grad[0, 2].float().norm()) > 0
    assert float(b.grad[1, n - 1].float().norm()) > 0
    monkeypatch.setenv("CLIPX_MAXSIM_FUSED", "0")
    a2 = a.detach().clone().requires_grad_(True)
    b2 = b.detach().clone().requires_grad_(True)
    assert not LS._MaxSimFused.applies(a2, b2)
    if (ni * q) % 8 == 0 and (nt * n) % 8 == 0 and nt % 8 == 0:
        out2 = LS.compute_colbert_similarity(a2, b2)
        assert float((out2 - out).detach().abs().max()) < 2e-2       # there S is rounded to bf16 before the max


@pytest.mark.parametrize("q,k", [(17, 3), (49, 1)])
def test_ties_go_to_the_first_token(q, k):
    """Image k (columns k q .. (k + 1) q - 1 straddle column 64: two slots, two partials) holds ONE vector q times.  Every
    maximum over it is a q-way tie: the whole gradient of the image sits on token 0 (the smaller column inside a slot, the
    first partial across slots, like torch.max), and its logits are those of an image that holds the vector once."""
    ni, nt, n, e = 8, 6, 9, 128
    assert k * q < 64 < (k + 1) * q - 1
    ti, tt = R.tokens(ni, q, nt, n, e)
    ti[k, :] = ti[k, 0].clone()
    a = ti.to(DEV).bfloat16().requires_grad_(True)
    b = tt.to(DEV).bfloat16().requires_grad_(True)
    assert LS._MaxSimFused.applies(a, b)
    out = LS.compute_colbert_similarity(a, b)
    gout = torch.randn(nt, ni, generator=torch.Generator().manual_seed(q)).to(DEV)
    out.backward(gout)
    ga = a.grad.float()
    assert float(ga[k, 1:].abs().max()) == 0.0 and float(ga[k, 0].norm()) > 0
    ref = R.einsum_ref(a.detach().float(), b.detach().float())              # [nt, ni]
    assert float((out - ref).detach().abs().max()) < 2e-5
    once = (b.detach().float() @ a.detach().float()[k, 0]).unsqueeze(1)     # [nt, 1, n] -> the image with the token once
    want = once.sum(-1) / ((once != 0).float().sum(-1) + 1e-8)
    assert float((out[:, k:k + 1] - want).detach().abs().max()) < 2e-5
    # the other images are untouched by the duplicate rows
    others = [i for i in range(ni) if i != k]
    assert float(ga[others].abs().sum()) > 0


def test_similarity_matrix_is_never_written():
    """64 images x 49 tokens against 64 x 77 distinct text rows: S would be 4928 x 3136 bf16 = 30.9 MB.  The forward's peak rise
    stays under half of that; by the layouts it is partials 2 x 64 x 5120 x 6 B = 3.9 MB + maxvT / argT 64 x 5120 x 6 B = 2.0 MB +
    packed text 1.3 MB + row tables: under 10 MB."""
    ni, q, nt, n, e = 64, 49, 64, 77, 128
    g = torch.Generator().manual_seed(9)
    a = torch.nn.functional.normalize(torch.randn(ni, q, e, generator=g), dim=-1).to(DEV).bfloat16().requires_grad_(True)
    b = torch.nn.functional.normalize(torch.randn(nt, n, e, generator=g), dim=-1).to(DEV).bfloat16().requires_grad_(True)
    s_bytes = nt * n * ni * q * 2
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = LS.compute_colbert_similarity(a, b)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    print(f"forward peak rise {rise / 1e6:.2f} MB (S: {s_bytes / 1e6:.1f} MB)")
    assert out.shape == (nt, ni)
    assert rise < s_bytes // 2, rise
    assert rise < 10e6, rise
    ref = R.einsum_ref(a.detach().float(), b.detach().float())
    assert float((out - ref).detach().abs().max()) < 2e-5


# (5 * 49) % 8 != 0: three zero images are appended to the only image chunk; (20, 49): chunks of 8 images, the last one half padding
SCORE_SHAPES = [(5, 49, 7, 20, 128), (8, 17, 6, 9, 128), (20, 49, 7, 20, 128), (5, 24, 6, 9, 128)]
# images per chunk (a multiple of 8 / gcd(q, 8)) and packed rows per text chunk of the shrunk plan
SCORE_SHRUNK = {(5, 49, 7, 20, 128): (8, 16), (8, 17, 6, 9, 128): (8, 16), (20, 49, 7, 20, 128): (8, 16), (5, 24, 6, 9, 128): (2, 16)}


@pytest.mark.parametrize("ni,q,nt,n,e", SCORE_SHAPES)
def test_score_fold_below_64_tokens(ni, q, nt, n, e, monkeypatch):
    """tests/test_late_interaction_gpu.py::test_fold_kernel_vs_reference_arithmetic below 64 tokens per image:
    `clipx_maxsim_score_fold` runs, 2e-5 against the einsum, and shrunk chunk limits (>= 2 text chunks; >= 2 image chunks where
    the image count has room for two alignment units) give bit-equal scores."""
    ti, tt = R.tokens(ni, q, nt, n, e)
    a, b = ti.to(DEV).bfloat16(), tt.to(DEV).bfloat16()
    assert ops.maxsim_fused_applies(a, b)
    calls = []
    fold = ops.maxsim_score_fold
    monkeypatch.setattr(ops, "maxsim_score_fold", lambda *args: (calls.append(args[:2]), fold(*args))[1])
    scores = ops.maxsim_scores(a, b, None, 0.0, 1.0)
    assert scores.shape == (ni, nt) and scores.dtype == torch.float32
    assert len(calls) == 1 and calls[0] == (nt, ni)
    ref = R.einsum_ref(a.float(), b.float())                     # [nt, ni]
    err = float((scores - ref.t()).abs().max())
    print(f"fold ({ni},{q},{nt},{n},{e}): max |scores - ref^T| = {err:.3e}")
    assert err < 2e-5, err
    cu, _ = ops.maxsim_pack_text(b)
    cu = cu.cpu().tolist()
    ci, rows = SCORE_SHRUNK[(ni, q, nt, n, e)]
    R.shrink(monkeypatch, q, e, ci, rows)
    image_chunks, text_chunks = ops.plan_maxsim_chunks(ni, q, e, cu, ops.MAXSIM_PARTIAL_BYTES)
    assert len(text_chunks) >= 2
    assert len(image_chunks) == (ni + ci - 1) // ci
    if (ni * q) % 8:
        assert image_chunks[-1][2] > image_chunks[-1][1] - image_chunks[-1][0]      # zero images behind the last real one
    del calls[:]
    chunked = ops.maxsim_scores(a, b, None, 0.0, 1.0)
    assert len(calls) == len(image_chunks) * len(text_chunks)
    assert torch.equal(chunked, scores)
    G = torch.randn(ni, nt, generator=torch.Generator().manual_seed(6)).to(DEV)
    want = 14.0 * (0.3 * G + 0.7 * ref.t())
    assert float((ops.maxsim_scores(a, b, G, 0.3, 14.0) - want).abs().max()) < 14.0 * 2e-5


def test_fused_route_through_a_49_token_model(monkeypatch):
    """ViT-q49-test-colxlip (112 px / patch 16: 49 image tokens, embed dim 128) in bf16: a training step through ColClipLoss and
    `get_logits` under no_grad both take the fused route.  The step against the oracle's `colxlip_loss_and_grads` with the bf16
    bounds of tests/test_model_gpu.py::test_colxlip_model_vs_oracle; the scores with the bounds of
    tests/test_late_interaction_gpu.py::test_fused_route_through_a_model."""
    from colxlip_amd.loss import ColClipLoss
    sd = R.model_state(Q49)
    image, text = O.synthetic_batch(Q49, 8, seed=21)
    ref_out, ref_res, ref_grads = O.colxlip_loss_and_grads(sd, image, text, Q49, alpha=0.4)
    gemms, folds = [], []
    gemm, fold = ops.maxsim_gemm, ops.maxsim_score_fold
    monkeypatch.setattr(ops, "maxsim_gemm", lambda *args: (gemms.append(args[2:4]), gemm(*args))[1])
    monkeypatch.setattr(ops, "maxsim_score_fold", lambda *args: (folds.append(args[:3]), fold(*args))[1])
    model = R.build_model(Q49_MODEL, sd, "bf16")
    model.train()
    model.zero_grad(set_to_none=True)
    out = model(image.to(DEV), text.to(DEV))
    assert out["token_image_features"].shape == (8, 49, 128) and out["token_image_features"].dtype == torch.bfloat16
    res = ColClipLoss(alpha=0.4)(**out, output_dict=True)
    res["total_loss"].backward()
    assert gemms == [(8, 49)] and not folds
    ftol, ltol, gtol = 4e-2, 6e-2, 0.2
    for k in ("image_features", "text_features", "token_image_features", "token_text_features"):
        assert float((out[k].detach().float().cpu() - ref_out[k]).abs().max()) < ftol, k
    for k in ("global_contrastive_loss", "token_contrastive_loss", "total_loss"):
        print(f"q49 model {k}: {float(res[k].detach()):.5f} (oracle {float(ref_res[k]):.5f})")
        assert abs(float(res[k].detach()) - float(ref_res[k])) < ltol, k
    grads = {k: p.grad.detach().float().cpu() for k, p in model.named_parameters() if p.grad is not None}
    for k in sd:
        ref = ref_grads[k]
        if float(ref.norm()) > 1e-4:
            rel = float((grads[k] - ref).norm() / (ref.norm() + 1e-8))
            assert rel < gtol, (k, rel)
    # get_logits without grad: ops.maxsim_scores on the fused route
    model.eval()
    del gemms[:]
    with torch.no_grad():
        li, lt = model.get_logits(image.to(DEV), text.to(DEV), alpha=0.5)
        found = model.encode_image(image.to(DEV), normalize=True), model.encode_text(text.to(DEV), normalize=True)
    assert folds == [(8, 8, 49)] and gemms == [(8, 49)] and torch.equal(lt, li.T)
    scale = float(model.logit_scale.detach().exp())
    from colxlip_amd.train import similarity_matrix
    G = similarity_matrix(found[0][0], found[1][0])
    same = float((ops.maxsim_scores(found[0][1], found[1][1], G, 0.5, scale) -
                  ops._maxsim_scores_general(found[0][1], found[1][1], G, 0.5, scale, torch.empty_like(G))).abs().max())
    print(f"q49 model: fused route vs fp32 arithmetic on the same bf16 tokens: {same:.3e}")
    assert same < scale * 2e-5, same
    fwd = O.colxlip_forward(sd, image, text, Q49)
    want = fwd["logit_scale"] * (0.5 * fwd["image_features"] @ fwd["text_features"].t()
                                 + 0.5 * O.colbert_similarity(fwd["token_image_features"], fwd["token_text_features"]).t())
    err = float((li.float().cpu() - want).abs().max())
    print(f"q49 model: max |bf16 get_logits - fp32 oracle| = {err:.3e}")
    assert err < 2e-2, err
