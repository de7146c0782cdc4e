"""Late-interaction retrieval for ColXLIP on the GPU: the forward-only MaxSim scorer (`ops.maxsim_scores`: the MaxSim GEMM's slot
partials folded straight into the dense score matrix by `clipx_maxsim_score_fold`), `ColXLIP.get_logits`, and `train.evaluate`
with a ColXLIP model (`--alpha`, `--evaluate-as-original-clip`).

Pinning: the scorer against the reference's arithmetic (loss.py:20-46) in fp32 on the same values, and against
tests/golden/late_interaction.npz (the reference's own `compute_colbert_similarity` and `compute_retrieval`, executed by
tests/golden/make_golden_late_interaction.py); the model and the evaluation loop against the CPU oracle."""
import json
import logging
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from colxlip_amd import ops  # noqa: E402
from colxlip_amd import train as TR  # noqa: E402
from colxlip_amd.data import synthetic_retrieval_split  # noqa: E402
from colxlip_amd.main import main  # noqa: E402
from colxlip_amd.params import parse_args  # noqa: E402
from oracle import clip_oracle as O  # noqa: E402
from tests import late_interaction_ref as R  # noqa: E402

DEV = "cuda"
MODEL = "ViT-small-test-colxlip"
CFG = O.ClipCfg(embed_dim=64, image_size=64, patch_size=16, vision_width=128, vision_layers=2,
                context_length=77, vocab_size=1024, text_width=128, text_heads=2, text_layers=2)
Q64_MODEL = "ViT-q64-test-colxlip"
Q64 = O.ClipCfg(embed_dim=128, image_size=128, patch_size=16, vision_width=128, vision_layers=2,
                context_length=77, vocab_size=1024, text_width=128, text_heads=2, text_layers=2)

# (ni, q, nt, n, e): slots never straddle an image, last slot partly filled / a boundary inside a slot, 3 slots per image /
# up to 5 slots per image and a sample of 77 distinct rows (a second lane pass) / an image count the GEMM alignment
# ((ni * q) % 8 == 0) does not take: one zero image is appended
FUSED_SHAPES = [(5, 64, 6, 9, 128), (4, 100, 7, 7, 256), (6, 196, 9, 77, 128), (5, 100, 7, 7, 256)]
# images per chunk and packed rows per text chunk of the shrunk plan
SHRUNK = {(5, 64, 6, 9, 128): (2, 16), (4, 100, 7, 7, 256): (2, 16), (6, 196, 9, 77, 128): (4, 96), (5, 100, 7, 7, 256): (2, 16)}


@pytest.mark.parametrize("ni,q,nt,n,e", FUSED_SHAPES)
def test_fold_kernel_vs_reference_arithmetic(ni, q, nt, n, e, monkeypatch):
    """The fused route (MaxSim GEMM partials -> clipx_maxsim_score_fold) against the reference's arithmetic in fp32 on the same bf16
    values, bound 2e-5 (the fused forward's bound on tok, tests/test_model_gpu.py:611); image-major output, checked element
    [k, m] against ref[m, k]; then once more with the chunk limits shrunk (>= 2 image chunks, >= 2 text chunks): bit-equal."""
    ti, tt = R.tokens(ni, q, nt, n, e)
    a, b = ti.to(DEV).bfloat16(), tt.to(DEV).bfloat16()
    assert ops.maxsim_fused_applies(a, b)
    calls = []
    fold = ops.maxsim_score_fold
    monkeypatch.setattr(ops, "maxsim_score_fold", lambda *args: (calls.append(args[:2]), fold(*args))[1])
    scores = ops.maxsim_scores(a, b, None, 0.0, 1.0)
    assert scores.shape == (ni, nt) and scores.dtype == torch.float32
    assert len(calls) == 1
    ref = R.einsum_ref(a.float(), b.float())                     # [nt, ni]
    err = max(abs(float(scores[k, m]) - float(ref[m, k])) for k in range(ni) for m in range(nt))
    print(f"fold ({ni},{q},{nt},{n},{e}): max |scores[k,m] - ref[m,k]| = {err:.3e}")
    assert err < 2e-5, err
    # packed rows: the single-row sample and the 'no duplicate' sample are what they are meant to be
    cu, _ = ops.maxsim_pack_text(b)
    cu = cu.cpu().tolist()
    assert cu[nt] - cu[nt - 1] == 1 and cu[3] - cu[2] == n
    ci, rows = SHRUNK[(ni, q, nt, n, e)]
    R.shrink(monkeypatch, q, e, ci, rows)
    image_chunks, text_chunks = ops.plan_maxsim_chunks(ni, q, e, cu, ops.MAXSIM_PARTIAL_BYTES)
    assert len(image_chunks) >= 2 and len(text_chunks) >= 2
    assert text_chunks[-1][3] - text_chunks[-1][2] < max(r1 - r0 for _, _, r0, r1 in text_chunks)
    if ni % ci:
        assert image_chunks[-1][1] - image_chunks[-1][0] < ci
    del calls[:]
    chunked = ops.maxsim_scores(a, b, None, 0.0, 1.0)
    assert len(calls) == len(image_chunks) * len(text_chunks)
    assert torch.equal(chunked, scores)


def test_combine_with_global_similarities():
    """scores = scale * (alpha * G + (1 - alpha) * tok^T) with random G; alpha = 1 is scale * G bit for bit."""
    ni, q, nt, n, e = 5, 64, 6, 9, 128
    ti, tt = R.tokens(ni, q, nt, n, e)
    a, b = ti.to(DEV).bfloat16(), tt.to(DEV).bfloat16()
    G = torch.randn(ni, nt, generator=torch.Generator().manual_seed(5)).to(DEV)
    scale = 14.0
    tok_t = ops.maxsim_scores(a, b, None, 0.0, 1.0)             # [ni, nt] = tok^T
    for alpha in (0.0, 0.3, 1.0):
        got = ops.maxsim_scores(a, b, G, alpha, scale)
        want = scale * (alpha * G + (1 - alpha) * tok_t)
        rel = float(((got - want).abs() / want.abs().clamp_min(1e-30)).max())
        print(f"combine alpha={alpha}: max relative difference {rel:.3e}")
        assert rel <= 1e-6, (alpha, rel)
    assert torch.equal(ops.maxsim_scores(a, b, G, 1.0, scale), scale * G)
    out = torch.full((ni, nt), float("nan"), device=DEV)
    assert ops.maxsim_scores(a, b, G, 0.3, scale, out=out) is out and torch.equal(out, ops.maxsim_scores(a, b, G, 0.3, scale))


@pytest.mark.parametrize("dtype,ni,q,nt,n,e", [(torch.float32, 5, 16, 7, 20, 64), (torch.bfloat16, 5, 49, 7, 20, 64)])
def test_general_route(dtype, ni, q, nt, n, e, monkeypatch):
    """fp32 tokens, and bf16 tokens with q < 64: fp32 arithmetic on gemm_f32 + maxsim_reduce + masked_mean, 2e-5 against the einsum
    reference on the same values (bf16 inputs are cast up: the same numbers, fp32 arithmetic); chunked = unchunked."""
    ti, tt = R.tokens(ni, q, nt, n, e)
    a, b = ti.to(DEV).to(dtype), tt.to(DEV).to(dtype)
    assert not ops.maxsim_fused_applies(a, b)
    monkeypatch.setattr(ops, "maxsim_score_fold", lambda *args: pytest.fail("the fused route ran"))
    scores = ops.maxsim_scores(a, b, None, 0.0, 1.0)
    assert scores.shape == (ni, nt)
    ref = R.einsum_ref(a.float(), b.float())
    err = float((scores - ref.t()).abs().max())
    print(f"general route {dtype}: max error {err:.3e}")
    assert err < 2e-5, err
    G = torch.randn(ni, nt, generator=torch.Generator().manual_seed(6)).to(DEV)
    want = 14.0 * (0.3 * G + 0.7 * ref.t())
    got = ops.maxsim_scores(a, b, G, 0.3, 14.0)
    assert float((got - want).abs().max()) < 14.0 * 2e-5
    monkeypatch.setattr(ops, "MAXSIM_GENERAL_BYTES", 4 * n * 2 * q)             # 2 images x 1 sample per chunk
    assert float((ops.maxsim_scores(a, b, G, 0.3, 14.0) - got).abs().max()) < 1e-5


def test_colxlip_get_logits_matches_oracle():
    """ColXLIP.get_logits on 6 images x 9 texts against the oracle's towers + colbert_similarity, bound 1e-4 (that of
    test_clip_get_logits_matches_oracle): without grad (ops.maxsim_scores) and with grad (the differentiable pieces)."""
    sd = R.model_state(CFG)
    model = R.build_model(MODEL, sd, "fp32")
    image, text = O.synthetic_batch(CFG, 9, seed=31)
    image = image[:6]
    ref = O.colxlip_forward(sd, image, text, CFG)
    glob = ref["image_features"] @ ref["text_features"].t()
    tok = O.colbert_similarity(ref["token_image_features"], ref["token_text_features"])      # [9, 6]
    scale = ref["logit_scale"]

    def want(alpha):
        return scale * (alpha * glob + (1 - alpha) * tok.t())

    assert model.alpha == 0.5
    with torch.no_grad():
        li, lt = model.get_logits(image.to(DEV), text.to(DEV))
        l3, _ = model.get_logits(image.to(DEV), text.to(DEV), alpha=0.3)
        l1, _ = model.get_logits(image.to(DEV), text.to(DEV), alpha=1.0)
    assert li.shape == (6, 9) and torch.equal(lt, li.T)
    for got, alpha in ((li, 0.5), (l3, 0.3), (l1, 1.0)):
        err = float((got.cpu() - want(alpha)).abs().max())
        print(f"get_logits (no grad) alpha={alpha}: max error {err:.3e}")
        assert err < 1e-4, (alpha, err)
    gi, gt = model.get_logits(image.to(DEV), text.to(DEV))
    assert gi.requires_grad and torch.equal(gt, gi.T)
    assert float((gi.detach().cpu() - want(0.5)).abs().max()) < 1e-4
    model.zero_grad(set_to_none=True)
    gi.sum().backward()
    heads = dict(model.named_parameters())
    assert heads["text_token_layer.1.weight"].grad is not None and float(heads["text_token_layer.1.weight"].grad.abs().max()) > 0
    assert heads["vision_token_layer.1.weight"].grad is not None and model.logit_scale.grad is not None
    g3, _ = model.get_logits(image.to(DEV), text.to(DEV), alpha=0.3)
    assert float((g3.detach().cpu() - want(0.3)).abs().max()) < 1e-4
    g1, _ = model.get_logits(image.to(DEV), text.to(DEV), alpha=1.0)
    assert float((g1.detach().cpu() - scale * glob).abs().max()) < 1e-4
    out = model(image[:2].to(DEV), text[:2].to(DEV))             # forward() and its key set are what they were
    assert sorted(out) == ["image_features", "logit_scale", "text_features", "token_image_features", "token_text_features"]


# ------------------------------------------------------------------------------------------------ evaluate() end to end
def _args(model_name, precision, extra=()):
    a = parse_args(["--model", model_name, "--dataset-type", "synthetic", "--precision", precision, "--batch-size", "8", *extra])
    a.rank, a.local_rank, a.world_size, a.distributed, a.device = 0, 0, 1, False, "cuda"
    a.save_logs, a.wandb = False, False
    return a


def _rows(split):
    """the split's id dictionaries in row indices of the encoded matrices (reference train.py:429-454)"""
    _, img, img2txt_dict, txt2img_dict = split
    img_ids = torch.cat([i for _, i in img.dataloader])
    row_of = {int(old): row for row, old in enumerate(img_ids.tolist())}
    img2txt = {row_of[i]: list(caps) for i, caps in img2txt_dict.items()}
    txt2img = {c: row_of[imgs[0]] for c, imgs in txt2img_dict.items()}
    return txt2img, img2txt


def _ambiguous(scores, txt2img, img2txt, gap=1e-3):
    """per direction: (queries with a competitor within `gap` of the target, such competitors in all, queries), in the given scores
    [n_img, n_txt].  The target of a caption is its image.  The target of an image is its best-scoring caption: the reference
    takes the smallest rank over an image's captions (train.py:488-493), which is the number of OTHER images' captions above
    that best one -- a caption of the image itself is never a competitor, and one of another image changes the rank only by
    crossing the best caption's score (with every score moved by at most d, only those within 2 d of it can)."""
    n_img, n_txt = scores.shape
    t_q = t_c = i_q = i_c = 0
    for c in range(n_txt):
        col = scores[:, c]
        close = int(((col - col[txt2img[c]]).abs() <= gap).sum()) - 1
        t_q += close > 0
        t_c += close
    for i in range(n_img):
        row = scores[i]
        other = torch.ones(n_txt, dtype=torch.bool)
        other[img2txt[i]] = False
        close = int(((row[other] - row[img2txt[i]].max()).abs() <= gap).sum())
        i_q += close > 0
        i_c += close
    return {"text_to_image": (t_q, t_c, n_txt), "image_to_text": (i_q, i_c, n_img)}


def _check_against_oracle_scores(got, prefix, oracle_scores, txt2img, img2txt, want=None):
    """Metrics against those of the oracle's own scores: a recall may differ by a / n, a = the queries whose target has a
    competitor within 1e-3 in the oracle's scores (ten times the score bound); the mean rank by (such competitors) / n.
    More than 10 % such queries marks the input as ill-conditioned: that fails, it is no tolerance."""
    if want is None:
        want = O.retrieval_metrics(oracle_scores, txt2img, img2txt)
    amb = _ambiguous(oracle_scores, txt2img, img2txt)
    for direction, (a, comp, n) in amb.items():
        print(f"{prefix}{direction}: {a} of {n} queries with a competitor within 1e-3 ({comp} competitors)")
        assert a <= 0.1 * n, (direction, a, n)
        for k in ("R@1", "R@5", "R@10"):
            name = f"{direction}_{k}"
            assert abs(got[prefix + name] - want[name]) <= a / n + 1e-9, (name, got[prefix + name], want[name], a)
        name = f"{direction}_mean_rank"
        assert abs(got[prefix + name] - want[name]) <= comp / n + 1e-5, (name, got[prefix + name], want[name])


@pytest.fixture(scope="module")
def coco_case():
    """The 24 x 5 split, ViT-small-test-colxlip weights, and the oracle's global and token similarities on it (computed once)."""
    sd = R.model_state(CFG)
    split = synthetic_retrieval_split(24, 5, CFG.image_size, CFG.context_length, CFG.vocab_size, seed=99, device="cuda", batch_size=7)
    txt, img, _, _ = split
    images = torch.cat([x for x, _ in img.dataloader]).float().cpu()
    texts = torch.cat([t for t, _ in txt.dataloader]).cpu()
    with torch.no_grad():
        ref = O.colxlip_forward(sd, images, texts, CFG)
        glob = ref["image_features"] @ ref["text_features"].t()                                     # [24, 120]
        tok = O.colbert_similarity(ref["token_image_features"], ref["token_text_features"])         # [120, 24]
    scale = ref["logit_scale"]
    txt2img, img2txt = _rows(split)
    return {"sd": sd, "split": split, "images": images, "texts": texts, "txt2img": txt2img, "img2txt": img2txt,
            "img_ids": torch.cat([i for _, i in img.dataloader]),
            "scores": lambda alpha: scale * (alpha * glob + (1 - alpha) * tok.t())}


def test_evaluate_colxlip_fp32(coco_case, caplog, tmp_path):
    """evaluate() with a ColXLIP model, --alpha 0.5, fp32: (a) the score matrix within 1e-4 of the oracle's
    scale * (0.5 G + 0.5 colbert^T); (b) the metrics ARE the reference's metric arithmetic on the product's own scores (id
    remapping, prefixes, counts, results.jsonl, mode restore, cadence); (c) the metrics against the oracle's own scores."""
    c = coco_case
    split = c["split"]
    txt, img, _, _ = split
    model = R.build_model(MODEL, c["sd"], "fp32")
    model.train()
    args = _args(MODEL, "fp32", ["--alpha", "0.5", "--epochs", "3", "--val-frequency", "2"])
    args.save_logs, args.checkpoint_path = True, str(tmp_path)
    scores, img_ids, cap_ids = TR.late_interaction_scores(model.eval(), txt.dataloader, img.dataloader, torch.device("cuda"),
                                                          torch.float32, alpha=0.5)
    model.train()
    assert scores.shape == (24, 120) and torch.equal(img_ids, c["img_ids"]) and cap_ids.tolist() == list(range(120))
    err = float((scores.cpu() - c["scores"](0.5)).abs().max())
    print(f"evaluate fp32: max |scores - oracle| = {err:.3e}")
    assert err < 1e-4, err
    with caplog.at_level(logging.INFO):
        assert TR.evaluate(model, {"retrieval_coco": split}, 1, args) == {}       # not on the cadence, not the last epoch
        got = TR.evaluate(model, {"retrieval_coco": split}, 2, args)
    assert model.training
    assert sum(r.getMessage().startswith("Eval Epoch: 2 ") for r in caplog.records) == 1
    assert got["epoch"] == 2 and got["retrieval_coco_num_text_samples"] == 120 and got["retrieval_coco_num_image_samples"] == 24
    own = O.retrieval_metrics(scores.cpu(), c["txt2img"], c["img2txt"])
    assert set(got) == {"epoch", "retrieval_coco_num_text_samples", "retrieval_coco_num_image_samples"} | {"retrieval_coco_" + k for k in own}
    for name, val in own.items():
        assert abs(got["retrieval_coco_" + name] - val) < 1e-6, (name, got["retrieval_coco_" + name], val)
    with open(os.path.join(tmp_path, "results.jsonl")) as f:
        rows = [json.loads(line) for line in f]
    assert len(rows) == 1 and rows[0] == got
    _check_against_oracle_scores(got, "retrieval_coco_", c["scores"](0.5), c["txt2img"], c["img2txt"])
    args.rank = 1
    assert TR.evaluate(model, {"retrieval_coco": split}, 2, args) == {}           # master only


def test_evaluate_colxlip_bf16(coco_case):
    """bf16 towers and tokens feed rounded features into the same ranking: the slack of test_evaluate_matches_oracle_pipeline."""
    c = coco_case
    model = R.build_model(MODEL, c["sd"], "bf16")
    args = _args(MODEL, "bf16", ["--alpha", "0.5"])
    got = TR.evaluate(model, {"retrieval_coco": c["split"]}, 1, args)
    want = O.retrieval_metrics(c["scores"](0.5), c["txt2img"], c["img2txt"])
    for name, val in want.items():
        mine = got["retrieval_coco_" + name]
        if "R@" in name:
            assert abs(mine - val) <= 0.05, (name, mine, val)
        else:
            assert abs(mine - val) <= 0.08 * val + 1.0, (name, mine, val)


def test_evaluate_as_original_clip(coco_case):
    """--evaluate-as-original-clip scores a ColXLIP model on its global features only (the reference's `original_clip` mode):
    the existing global-only oracle's metrics, and key for key those of --alpha 1.0."""
    c = coco_case
    model = R.build_model(MODEL, c["sd"], "fp32")
    got = TR.evaluate(model, {"retrieval_coco": c["split"]}, 1, _args(MODEL, "fp32", ["--alpha", "0.5", "--evaluate-as-original-clip"]))
    alpha1 = TR.evaluate(model, {"retrieval_coco": c["split"]}, 1, _args(MODEL, "fp32", ["--alpha", "1.0"]))
    assert got == alpha1 and len(got) == 13
    _, _, img2txt_dict, txt2img_dict = c["split"]
    want = O.retrieval_eval(c["sd"], c["images"], c["img_ids"], c["texts"], img2txt_dict, txt2img_dict, CFG)
    _check_against_oracle_scores(got, "retrieval_coco_", c["scores"](1.0), c["txt2img"], c["img2txt"], want=want)
    half = TR.evaluate(model, {"retrieval_coco": c["split"]}, 1, _args(MODEL, "fp32", ["--alpha", "0.5"]))
    assert half != got                                          # the token term does move this split's metrics


def test_fused_route_through_a_model(monkeypatch):
    """ViT-q64-test-colxlip (128 px / patch 16: 64 image tokens, embed dim 128) in bf16 takes the fused route inside evaluate();
    its scores within 2e-2 (the bf16-vs-fp32 MaxSim bound, tests/test_model_gpu.py:572) of the fp32 run of the same model."""
    sd = R.model_state(Q64)
    split = synthetic_retrieval_split(16, 3, Q64.image_size, Q64.context_length, Q64.vocab_size, seed=7, device="cuda", batch_size=8)
    txt, img, _, _ = split
    calls = []
    fold = ops.maxsim_score_fold
    monkeypatch.setattr(ops, "maxsim_score_fold", lambda *args: (calls.append(args[:2]), fold(*args))[1])
    m16 = R.build_model(Q64_MODEL, sd, "bf16")
    got = TR.evaluate(m16, {"retrieval_coco": split}, 1, _args(Q64_MODEL, "bf16", ["--alpha", "0.5"]))
    assert len(calls) == 1 and calls[0] == (48, 16)
    assert got["retrieval_coco_num_text_samples"] == 48 and 0.0 <= got["retrieval_coco_text_to_image_R@1"] <= 1.0
    s16, _, _ = TR.late_interaction_scores(m16.eval(), txt.dataloader, img.dataloader, torch.device("cuda"), TR.get_input_dtype("bf16"), alpha=0.5)
    assert len(calls) == 2
    m32 = R.build_model(Q64_MODEL, sd, "fp32").eval()
    s32, _, _ = TR.late_interaction_scores(m32, txt.dataloader, img.dataloader, torch.device("cuda"), torch.float32, alpha=0.5)
    assert len(calls) == 2                                      # fp32 tokens: the general route
    # the fused route against fp32 arithmetic on the bf16 model's own tokens (the general route): the fold bound, times the scale
    found = TR.encode_split(m16, txt.dataloader, img.dataloader, torch.device("cuda"), TR.get_input_dtype("bf16"), with_tokens=True)
    assert found[4].dtype == torch.bfloat16 and found[4].shape == (16, 64, 128) and found[5].shape == (48, 77, 128)
    scale = float(m16.logit_scale.exp())
    G = TR.similarity_matrix(found[0], found[2])
    same = float((ops.maxsim_scores(found[4], found[5], G, 0.5, scale) -
                  ops._maxsim_scores_general(found[4], found[5], G, 0.5, scale, torch.empty_like(G))).abs().max())
    print(f"q64 model: fused route vs fp32 arithmetic on the same bf16 tokens: {same:.3e}")
    assert same < scale * 2e-5, same
    err = float((s16 - s32).abs().max())
    print(f"q64 model: max |bf16 scores - fp32 scores| = {err:.3e}")
    assert err < 2e-2, err


def test_main_colxlip_with_retrieval(tmp_path, caplog):
    """main() trains a ColXLIP model for an epoch and evaluates it: one Eval Epoch line, one results.jsonl row."""
    argv = ["--model", MODEL, "--dataset-type", "synthetic", "--precision", "fp32", "--batch-size", "8", "--logs-dir", str(tmp_path),
            "--name", "li", "--retrieval-coco", "--val-num-samples", "16", "--epochs", "1", "--train-num-samples", "16"]
    with caplog.at_level(logging.INFO):
        assert main(argv) == 0
    assert sum(r.getMessage().startswith("Eval Epoch") for r in caplog.records) == 1
    with open(os.path.join(tmp_path, "li", "checkpoints", "results.jsonl")) as f:
        rows = [json.loads(line) for line in f]
    assert len(rows) == 1 and "retrieval_coco_text_to_image_R@1" in rows[0]


def test_scores_and_metrics_equal_reference_fixture(golden_dir):
    """The reference's own compute_colbert_similarity + compute_retrieval on a 6 x 10 gallery (tests/golden/late_interaction.npz):
    ops.maxsim_scores within 2e-5 of the stored scale * (0.7 G + 0.3 tok^T); compute_retrieval on them gives the stored metrics
    (a recall may differ by the share of queries with a competitor within 1e-3 in the stored scores)."""
    z = np.load(os.path.join(golden_dir, "late_interaction.npz"), allow_pickle=False)
    ti, tt = torch.from_numpy(z["token_image_features"]).to(DEV), torch.from_numpy(z["token_text_features"]).to(DEV)
    G = TR.similarity_matrix(torch.from_numpy(z["image_features"]).to(DEV), torch.from_numpy(z["text_features"]).to(DEV))
    tok_t = ops.maxsim_scores(ti, tt, None, 0.0, 1.0)
    assert float((tok_t.cpu() - torch.from_numpy(z["tok"]).t()).abs().max()) < 2e-5
    scores = ops.maxsim_scores(ti, tt, G, float(z["alpha"]), float(z["scale"]))
    stored = torch.from_numpy(z["scores"])
    assert scores.shape == stored.shape == (6, 10)
    err = float((scores.cpu() - stored).abs().max())
    print(f"reference fixture: max |scores - stored| = {err:.3e}")
    assert err < 2e-5, err
    owner = z["owner"].tolist()
    txt2img = {c: owner[c] for c in range(10)}
    img2txt = {i: [c for c in range(10) if owner[c] == i] for i in range(6)}
    remapped = TR.remap_indices(torch.from_numpy(z["img_ids"]), torch.from_numpy(z["cap_ids"]),
                                {int(z["img_ids"][i]): img2txt[i] for i in range(6)},
                                {c: [int(z["img_ids"][owner[c]])] for c in range(10)})
    assert remapped == (img2txt, txt2img)
    got = TR.compute_retrieval(scores, txt2img, img2txt)
    want = dict(zip([str(k) for k in z["metric_names"]], z["metric_values"].tolist()))
    assert list(got) == list(want)
    amb = _ambiguous(stored, txt2img, img2txt)
    for direction, (a, comp, n) in amb.items():
        assert a <= 0.1 * n, (direction, a, n)
        for name in want:
            if name.startswith(direction):
                slack = a / n if "R@" in name else comp / n + 1e-5 if "mean" in name else float(a > 0)
                assert abs(got[name] - want[name]) <= slack + 1e-9, (name, got[name], want[name])
