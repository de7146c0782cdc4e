"""The e4m3 token index on the GPU: `ops.maxsim_scores_fp8` (the MaxSim GEMM on the fp8 MFMA, `clipx_maxsim_gemm_fp8`) and
`LateInteractionIndex(token_dtype="fp8")`.

What the scorer computes is MaxSim of the DEQUANTISED tokens (`quant_tokens_e4m3` then `dequant_tokens_e4m3`): every product of
two e4m3 values is exact in fp32, so the only error against the reference arithmetic on those values is the fp32 summation,
as on the bf16 route.  Selections are compared EXACTLY (values bit for bit) with `search.topk_reference` on the dense matrix
`ops.maxsim_scores_fp8` builds over the same chunk boundaries."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from colxlip_amd import ops  # noqa: E402
from colxlip_amd import search as S  # noqa: E402
from colxlip_amd import train as TR  # noqa: E402
from colxlip_amd.search import LateInteractionIndex, topk_reference  # noqa: E402
from oracle import clip_oracle as O  # noqa: E402
from tests import late_interaction_ref as LR  # noqa: E402
from tests.late_interaction_ref import Q49  # noqa: E402

DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")


def _dequantised(x):
    """bf16 tokens -> the values the fp8 route scores, fp32 on the device"""
    return ops.dequant_tokens_e4m3(*ops.quant_tokens_e4m3(x))


def _count_calls(monkeypatch, *names):
    """{name: [calls]} of ops functions, which still run"""
    seen = {}
    for name in names:
        fn = getattr(ops, name)
        seen[name] = []
        monkeypatch.setattr(ops, name, lambda *a, _fn=fn, _log=seen[name], **kw: (_log.append(a), _fn(*a, **kw))[1])
    return seen


def _bits(t):
    return t.contiguous().view(torch.int32)


# ------------------------------------------------------------------------------------------------ 1. the scorer
# (ni, q, nt, n, e): the segment epilogue with an image boundary inside a 16-column block / the two-segment epilogue / the smallest
# q / more than 256 packed rows and more than 256 token columns: several tiles each way, a row tail and a column tail
FP8_SHAPES = [(5, 49, 7, 20, 256, False), (5, 80, 7, 20, 256, False), (9, 16, 6, 9, 256, False), (7, 64, 24, 20, 256, True)]


@pytest.mark.parametrize("ni,q,nt,n,e,distinct", FP8_SHAPES)
def test_fp8_scorer_vs_reference_arithmetic(ni, q, nt, n, e, distinct, monkeypatch):
    """`maxsim_scores_fp8` on bf16 inputs against the reference's arithmetic in fp64 on the dequantised operands.  The bound is
    measured beside it: the bf16 fused route on the same (bf16-exact) values against the same fp64 numbers; the fp8 error may be
    4 times that (sums over 128-wide instead of 32-wide steps) or 2e-5 (the bf16 route's own bound,
    tests/test_late_interaction_gpu.py), whichever is larger.

    Measured on an MI355X (max |scores - fp64|, fp8 route / bf16 route): (5,49,7,20,256) 1.21e-06 / 1.46e-08; (5,80,7,20,256)
    9.05e-07 / 1.74e-08; (9,16,6,9,256) 1.62e-06 / 1.39e-08; (7,64,24,20,256) 2.62e-06 / 1.82e-08.  Inside 2e-5, but the fp8 MFMA's
    sums are 50 to 150 times less accurate than the bf16 MFMA's."""
    a, b = (t.to(DEV).bfloat16() for t in LR.tokens(ni, q, nt, n, e, distinct=distinct))
    assert ops.maxsim_fp8_applies(a, b)
    seen = _count_calls(monkeypatch, "maxsim_gemm_fp8", "maxsim_gemm", "maxsim_reduce")
    scores = ops.maxsim_scores_fp8(a, b, None, 0.0, 1.0)
    assert scores.shape == (ni, nt) and scores.dtype == torch.float32
    assert len(seen["maxsim_gemm_fp8"]) == 1 and not seen["maxsim_gemm"] and not seen["maxsim_reduce"]
    R = seen["maxsim_gemm_fp8"][0][0].shape[0]
    if distinct:
        assert R > 256 and ni * q > 256 and R % 256 and (ni * q) % 256          # several tiles each way, with tails
    da, db = _dequantised(a), _dequantised(b)
    assert torch.equal(da.bfloat16().float(), da) and torch.equal(db.bfloat16().float(), db)
    ref = LR.einsum_ref(da.cpu().double(), db.cpu().double()).t()                  # [ni, nt] fp64
    err8 = float((scores.cpu().double() - ref).abs().max())
    bf16 = ops.maxsim_scores(da.bfloat16(), db.bfloat16(), None, 0.0, 1.0)       # the fused bf16 route on the same values
    assert len(seen["maxsim_gemm"]) == 1
    err16 = float((bf16.cpu().double() - ref).abs().max())
    print(f"fp8 scorer ({ni},{q},{nt},{n},{e}): max |scores - fp64| = {err8:.3e} (fp8 MFMA), {err16:.3e} (bf16 MFMA); "
          f"scores in {float(ref.min()):.3f} .. {float(ref.max()):.3f}, packed rows {R}")
    assert err8 <= max(4 * err16, 2e-5), (err8, err16)
    # how far the quantisation itself moves a score: reported, not bounded here
    moved = float((scores.cpu().double() - LR.einsum_ref(a.cpu().double(), b.cpu().double()).t()).abs().max())
    print(f"    |fp8 scores - fp64 on the bf16 tokens| = {moved:.3e}")


# images per chunk and packed rows per text chunk of the shrunk plan; 49 tokens: whole units of 8 images, the last chunk padded
SHRUNK = [(5, 80, 7, 20, 256, 2, 16), (9, 16, 6, 9, 256, 4, 16), (19, 49, 7, 20, 256, 8, 16)]


@pytest.mark.parametrize("ni,q,nt,n,e,ci,rows", SHRUNK)
def test_either_side_stored_and_chunked(ni, q, nt, n, e, ci, rows, monkeypatch):
    """(bytes, exp) images and (bytes, exp, cnt) texts give the scores of the on-the-fly call bit for bit, alone and together; so
    does the plan shrunk to >= 2 image chunks and >= 2 text chunks."""
    a, b = (t.to(DEV).bfloat16() for t in LR.tokens(ni, q, nt, n, e))
    G = torch.randn(ni, nt, generator=torch.Generator().manual_seed(5)).to(DEV)
    want = ops.maxsim_scores_fp8(a, b, G, 0.3, 14.0)
    img = ops.quant_tokens_e4m3(a)
    txt = ops.quant_tokens_e4m3(b) + (ops.maxsim_text_counts(b),)
    assert img[0].dtype == torch.uint8 and img[0].shape == (ni, q, e) and img[1].dtype == torch.int32 and img[1].shape == (ni, q)
    cu, R = ops.maxsim_pack_text(b)
    assert txt[2].dtype == torch.int32 and torch.equal(torch.cumsum(txt[2], 0).int(), cu[1:]) and int(txt[2][-1]) == 1
    for i_side, t_side in ((img, b), (a, txt), (img, txt), (list(img), list(txt))):
        assert ops.maxsim_fp8_applies(i_side, t_side)
        assert torch.equal(_bits(ops.maxsim_scores_fp8(i_side, t_side, G, 0.3, 14.0)), _bits(want))
    LR.shrink(monkeypatch, q, e, ci, rows, elem_bytes=1)
    image_chunks, text_chunks = ops.plan_maxsim_chunks(ni, q, e, cu.cpu().tolist(), ops.MAXSIM_PARTIAL_BYTES, elem_bytes=1)
    assert len(image_chunks) >= 2 and len(text_chunks) >= 2 and max(c for _, _, c in image_chunks) == ci
    if ni % ci:
        assert image_chunks[-1][1] - image_chunks[-1][0] < ci                                   # a shorter last chunk
    assert (image_chunks[-1][2] > image_chunks[-1][1] - image_chunks[-1][0]) == (q == 49)       # 49 tokens: zero images behind it
    seen = _count_calls(monkeypatch, "maxsim_gemm_fp8")
    for i_side, t_side in ((a, b), (img, txt)):
        del seen["maxsim_gemm_fp8"][:]
        assert torch.equal(_bits(ops.maxsim_scores_fp8(i_side, t_side, G, 0.3, 14.0)), _bits(want))
        assert len(seen["maxsim_gemm_fp8"]) == len(image_chunks) * len(text_chunks)


def test_fp8_combine_with_global_similarities():
    """scores = scale * (alpha * G + (1 - alpha) * tok^T) with random G; alpha = 1 is scale * G bit for bit, tokens unread."""
    ni, q, nt, n, e = 5, 80, 7, 20, 256
    a, b = (t.to(DEV).bfloat16() for t in LR.tokens(ni, q, nt, n, e))
    G = torch.randn(ni, nt, generator=torch.Generator().manual_seed(5)).to(DEV)
    scale = 14.0
    tok_t = ops.maxsim_scores_fp8(a, b, None, 0.0, 1.0)
    for alpha in (0.0, 0.3, 1.0):
        got = ops.maxsim_scores_fp8(a, b, G, alpha, scale)
        want = scale * (alpha * G + (1 - alpha) * tok_t)
        rel = float(((got - want).abs() / want.abs().clamp_min(1e-30)).max())
        print(f"fp8 combine alpha={alpha}: max relative difference {rel:.3e}")
        assert rel <= 1e-6, (alpha, rel)
    assert torch.equal(ops.maxsim_scores_fp8(a, b, G, 1.0, scale), scale * G)
    assert torch.equal(ops.maxsim_scores_fp8(None, None, G, 1.0, scale), scale * G)
    out = torch.full((ni, nt), float("nan"), device=DEV)
    assert ops.maxsim_scores_fp8(a, b, G, 0.3, scale, out=out) is out and torch.equal(out, ops.maxsim_scores_fp8(a, b, G, 0.3, scale))


@pytest.mark.parametrize("ni,q,nt,n,e,env", [(5, 16, 7, 20, 64, None), (5, 49, 7, 20, 320, None), (5, 49, 7, 20, 256, "0"),
                                             (5, 8, 7, 20, 256, None)])
def test_fp8_fallback_route(ni, q, nt, n, e, env, monkeypatch):
    """E = 64 (below 256), E = 320 (no multiple of 128), CLIPX_MAXSIM_FUSED=0 and q = 8 take the general fp32 route on the
    dequantised values: the fp8 GEMM op is not called, and the scores match the fp32 reference arithmetic on those values within
    2e-5, from bf16 inputs and from the stored forms alike."""
    if env is not None:
        monkeypatch.setenv("CLIPX_MAXSIM_FUSED", env)
    a, b = (t.to(DEV).bfloat16() for t in LR.tokens(ni, q, nt, n, e))
    assert not ops.maxsim_fp8_applies(a, b)
    monkeypatch.setattr(ops, "maxsim_gemm_fp8", lambda *args: pytest.fail("the fp8 GEMM ran"))
    seen = _count_calls(monkeypatch, "maxsim_reduce")
    scores = ops.maxsim_scores_fp8(a, b, None, 0.0, 1.0)
    assert scores.shape == (ni, nt) and len(seen["maxsim_reduce"]) >= 1
    ref = LR.einsum_ref(_dequantised(a), _dequantised(b)).t()
    err = float((scores - ref).abs().max())
    print(f"fp8 fallback ({ni},{q},{nt},{n},{e}, fused={env}): max error {err:.3e}")
    assert err < 2e-5, err
    img, txt = ops.quant_tokens_e4m3(a), ops.quant_tokens_e4m3(b) + (ops.maxsim_text_counts(b),)
    assert not ops.maxsim_fp8_applies(img, txt)
    assert torch.equal(_bits(ops.maxsim_scores_fp8(img, txt, None, 0.0, 1.0)), _bits(scores))
    G = torch.randn(ni, nt, generator=torch.Generator().manual_seed(6)).to(DEV)
    got = ops.maxsim_scores_fp8(a, b, G, 0.3, 14.0)
    assert float((got - 14.0 * (0.3 * G + 0.7 * ref)).abs().max()) < 14.0 * 2e-5


# ------------------------------------------------------------------------------------------------ 2. the index
@pytest.mark.parametrize("kind", ["image", "text"])
def test_fp8_index_equals_dense_route(kind, monkeypatch):
    """The scheme of test_search_gpu.py::test_index_equals_dense_route: 35 = 2 * 16 + 3 gallery items in chunks of 16, 19 queries in
    chunks of 8, q = 49, E = 256, 20-token captions, ids that are not the positions.  The reference: `ops.maxsim_scores_fp8` on the
    bf16 tokens of every (query chunk, gallery chunk) with the same boundaries, then `topk_reference`."""
    q, e, alpha, scale, n_gal, n_qry = 49, 256, 0.4, 13.5, 35, 19
    monkeypatch.setattr(LateInteractionIndex, "CHUNK_ITEMS", 16)
    monkeypatch.setattr(LateInteractionIndex, "QUERY_CHUNK", 8)
    n_img, n_txt = (n_gal, n_qry) if kind == "image" else (n_qry, n_gal)
    img_f, txt_f = LR.features(n_img, e, 1).to(DEV), LR.features(n_txt, e, 2).to(DEV)
    img_t, txt_t = LR.image_tokens(n_img, q, e, 3).to(DEV), LR.text_tokens(n_txt, 20, e, 4).to(DEV)
    gal_f, gal_t, qry_f, qry_t = (img_f, img_t, txt_f, txt_t) if kind == "image" else (txt_f, txt_t, img_f, img_t)
    ids = 1000 + 3 * torch.arange(n_gal)
    index = LateInteractionIndex(kind, alpha=alpha, scale=scale, device=DEV, token_dtype="fp8")
    index.add(gal_f[:20], gal_t[:20], ids=ids[:20])
    index.add(gal_f[20:], gal_t[20:].float(), ids=ids[20:])                     # fp32 tokens: bf16-exact here, cast back
    assert [c[1].shape[0] for c in index.chunks()] == [16, 16, 3]
    stored = index.chunks()[2][2]
    assert len(stored) == (3 if kind == "text" else 2) and stored[0].dtype == torch.uint8 and stored[0].shape == (3, gal_t.shape[1], e)
    assert all(t.dtype != torch.bfloat16 for store in (index._tok, index._tok_exp, index._tok_cnt) for t in store)
    seen = _count_calls(monkeypatch, "maxsim_gemm_fp8", "maxsim_gemm", "maxsim_reduce", "topk_merge")
    got5 = index.search(qry_f, qry_t, 5)
    n_calls = len(seen["maxsim_gemm_fp8"])
    got40 = index.search(qry_f, qry_t, 40)
    assert n_calls == 9 and len(seen["maxsim_gemm_fp8"]) == 18                  # 3 query chunks x 3 gallery chunks, one GEMM each
    assert not seen["maxsim_gemm"] and not seen["maxsim_reduce"]                # only the fp8 GEMM scored tokens
    merges = [(tuple(m[0].shape), m[1], m[2]) for m in seen["topk_merge"]]
    per_search = [(m[0][0] if kind == "image" else m[0][1], m[2]) for m in merges[:len(merges) // 2]]
    assert per_search == [(16, 0), (16, 16), (3, 32)] * 3 and all(m[1] == (1 if kind == "image" else 0) for m in merges)

    dense = torch.empty(n_img, n_txt, device=DEV)
    for q0 in range(0, n_qry, 8):
        q1 = min(n_qry, q0 + 8)
        for g0 in range(0, n_gal, 16):
            g1 = min(n_gal, g0 + 16)
            (i0, i1, t0, t1) = (g0, g1, q0, q1) if kind == "image" else (q0, q1, g0, g1)
            G = TR.similarity_matrix(img_f[i0:i1], txt_f[t0:t1])
            ops.maxsim_scores_fp8(img_t[i0:i1], txt_t[t0:t1], G, alpha, scale, out=dense[i0:i1, t0:t1])
    for got, k in ((got5, 5), (got40, 40)):
        want_v, want_p = topk_reference(dense.cpu(), k, 1 if kind == "image" else 0)
        assert got[0].is_cuda and got[1].is_cuda and got[1].dtype == torch.int64 and got[0].dtype == torch.float32
        want_ids = torch.where(want_p >= 0, ids[want_p.clamp(min=0).long()], torch.full_like(want_p, -1).long())
        assert torch.equal(got[1].cpu(), want_ids)
        assert torch.equal(_bits(got[0].cpu()), _bits(want_v))
        assert set(got[1].cpu().flatten().tolist()) <= set(ids.tolist()) | {-1}          # no item of the padded last chunk
    assert bool((got40[1][:, 35:] == -1).all()) and bool((got40[1][:, :35] >= 0).all())
    assert bool((got40[0][:, 35:] == -INF).all())


@pytest.mark.parametrize("kind", ["image", "text"])
def test_fp8_index_save_load_search_and_size(kind, tmp_path, monkeypatch):
    """A saved and reloaded fp8 index returns identical results; tokens.npy holds uint8, half the bytes of the default index's
    file; the stored token tensors take at most 0.51 of the bf16 index's (1/2 + 4 / (2 E) = 0.508 at E = 256 for the exponents;
    a text gallery's counts add 4 / (2 n E) = 0.0004)."""
    monkeypatch.setattr(LateInteractionIndex, "CHUNK_ITEMS", 16)
    monkeypatch.setattr(LateInteractionIndex, "IO_ITEMS", 7)
    e = 256
    if kind == "image":
        gal_t, qt = LR.image_tokens(35, 49, e, 3).to(DEV), LR.text_tokens(19, 20, e, 4).to(DEV)
    else:
        gal_t, qt = LR.text_tokens(35, 20, e, 3).to(DEV), LR.image_tokens(19, 49, e, 4).to(DEV)
    gal_f, qf = LR.features(35, e, 1).to(DEV), LR.features(19, e, 2).to(DEV)
    ids = torch.arange(35) * 2 + 5
    index = LateInteractionIndex(kind, alpha=0.4, scale=20.0, device=DEV, token_dtype="fp8").add(gal_f, gal_t, ids=ids)
    plain = LateInteractionIndex(kind, alpha=0.4, scale=20.0, device=DEV).add(gal_f, gal_t, ids=ids)
    ratio = index.token_bytes() / plain.token_bytes()
    print(f"stored token bytes, fp8 / bf16 ({kind} gallery): {index.token_bytes()} / {plain.token_bytes()} = {ratio:.4f}")
    assert ratio <= 0.51 and plain.token_bytes() == sum(t.numel() * 2 for t in plain._tok)
    first = index.search(qf, qt, 10)
    path = index.save(str(tmp_path / "fp8"))
    plain_path = plain.save(str(tmp_path / "bf16"))
    on_disk = np.load(os.path.join(path, "tokens.npy"), mmap_mode="r")
    assert on_disk.dtype == np.uint8 and 2 * on_disk.nbytes == np.load(os.path.join(plain_path, "tokens.npy"), mmap_mode="r").nbytes
    assert sorted(os.listdir(path)) == sorted(S._FILES + S._FP8_FILES[:2 if kind == "text" else 1])
    seen = _count_calls(monkeypatch, "quant_tokens_e4m3")
    back = LateInteractionIndex.load(path, device=DEV)
    assert not seen["quant_tokens_e4m3"]                                         # kept as saved, not quantised again
    assert back.token_dtype == "fp8" and len(back) == 35 and [c[1].shape[0] for c in back.chunks()] == [16, 16, 3]
    for (_, _, x), (_, _, y) in zip(index.chunks(), back.chunks()):
        assert len(x) == len(y) and all(u.is_cuda and u.dtype == v.dtype and torch.equal(u, v) for u, v in zip(y, x))
    again = back.search(qf, qt, 10)
    assert torch.equal(first[1], again[1]) and torch.equal(_bits(first[0]), _bits(again[0]))
    assert int(first[1].min()) >= 5
    # the quantised index ranks like the bf16 one on these features: reported
    ref = plain.search(qf, qt, 10)
    keep = np.mean([len(set(r.tolist()) & set(g.tolist())) / 10 for r, g in zip(ref[1].cpu(), first[1].cpu())])
    print(f"    top-10 overlap with the bf16 index {keep:.3f}, max |score difference| {float((ref[0] - first[0]).abs().max()):.3e}")


def test_fp8_peak_memory_does_not_grow_with_the_gallery(monkeypatch):
    """As test_search_gpu.py's for the fused route, on the fp8 route: 64 queries, k = 10, gallery chunks of 256 items, E = 256; what
    `search` allocates above what is live before it is the same, within 64 KiB, for 2 048 and 4 096 gallery items."""
    monkeypatch.setattr(LateInteractionIndex, "CHUNK_ITEMS", 256)
    e = 256
    qf, qt = LR.features(64, e, 2).to(DEV), LR.text_tokens(64, 20, e, 4).to(DEV)
    peaks = []
    for n in (2048, 4096):
        index = LateInteractionIndex("image", alpha=0.5, scale=10.0, device=DEV, token_dtype="fp8")
        index.add(LR.features(n, e, 1).to(DEV), LR.image_tokens(n, 16, e, 3).to(DEV))
        assert index.token_bytes() == n * 16 * (e + 4)
        index.search(qf, qt, 10)                                   # warm: library handles, kernel attributes
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        live = torch.cuda.memory_allocated()
        val, ids = index.search(qf, qt, 10)
        torch.cuda.synchronize()
        peaks.append(torch.cuda.max_memory_allocated() - live)
        assert int(ids.max()) < n and int(ids.min()) >= 0
        del index, val, ids
    print(f"fp8 search peak above live memory: {peaks[0]} B at 2048 items, {peaks[1]} B at 4096 items")
    assert abs(peaks[1] - peaks[0]) <= 64 * 1024, peaks


# ------------------------------------------------------------------------------------------------ 3. through a model and the CLI
NAME = "ViT-q49-test-colxlip"            # embed dim 128: below the kernel's 256, so the plumbing is checked on the fallback route


def _model():
    return LR.build_model(NAME, LR.model_state(Q49), "bf16").eval()


def test_fp8_search_through_a_model(monkeypatch):
    """add_images + search_texts and add_texts + search_images with token_dtype="fp8" against `topk_reference` of the dense fp8
    route on the features the model produced: one gallery chunk and one query chunk, so the tile is that matrix."""
    model = _model()
    image, text = O.synthetic_batch(Q49, 9, seed=31)
    image, text = image[:8].to(DEV, dtype=torch.bfloat16), text.to(DEV)
    img_f, img_t = LateInteractionIndex._encode(model, "image", image)
    txt_f, txt_t = LateInteractionIndex._encode(model, "text", text)
    assert img_t.shape == (8, 49, 128) and img_t.dtype == torch.bfloat16 and not ops.maxsim_fp8_applies(img_t, txt_t)
    scale = float(model.logit_scale.detach().exp())
    dense = ops.maxsim_scores_fp8(img_t, txt_t, TR.similarity_matrix(img_f, txt_f), model.alpha, scale)
    monkeypatch.setattr(ops, "maxsim_gemm", lambda *a: pytest.fail("the bf16 MaxSim GEMM ran"))
    images = LateInteractionIndex.from_model(model, "image", token_dtype="fp8")
    assert images.token_dtype == "fp8" and images.alpha == model.alpha
    images.add_images(model, image)
    assert len(images) == 8 and images.chunks()[0][2][0].dtype == torch.uint8 and images.chunks()[0][2][0].shape == (8, 49, 128)
    for k in (3, 8):
        val, ids = images.search_texts(model, text, k)
        want_v, want_p = topk_reference(dense.cpu(), k, 1)
        assert torch.equal(ids.cpu().int(), want_p) and torch.equal(_bits(val.cpu()), _bits(want_v))
    texts = LateInteractionIndex.from_model(model, "text", token_dtype="fp8").add_texts(model, text)
    assert len(texts.chunks()[0][2]) == 3 and texts.chunks()[0][2][2].shape == (9,)
    for k in (4, 12):
        val, ids = texts.search_images(model, image, k)
        want_v, want_p = topk_reference(dense.cpu(), k, 0)
        assert torch.equal(ids.cpu().int(), want_p) and torch.equal(_bits(val.cpu()), _bits(want_v))
    with pytest.raises(ValueError):
        images.search_images(model, image, 3)


def test_fp8_cli_save_then_load(tmp_path):
    """python -m colxlip_amd.search --index-dtype fp8 --save-index, then --load-index (which takes the dtype from meta.json):
    identical results.npz, and the directory holds the fp8 files."""
    model = _model()
    ckpt = str(tmp_path / "model.pt")
    torch.save({"state_dict": {k: v.detach().cpu() for k, v in model.state_dict().items()}}, ckpt)
    del model
    index_dir = str(tmp_path / "index")
    base = [sys.executable, *(["-s"] if sys.flags.no_user_site else []), "-c", LR.LAUNCHER, ROOT, "--model", NAME, "--dataset-type",
            "synthetic", "--precision", "bf16", "--batch-size", "16", "--retrieval-coco", "--val-num-samples", "16", "--alpha", "0.5",
            "--pretrained", ckpt, "--direction", "t2i", "--k", "5"]
    outs = []
    for extra in (["--index-dtype", "fp8", "--save-index", index_dir], ["--load-index", index_dir]):
        out = str(tmp_path / f"{len(outs)}.npz")
        done = subprocess.run(base + ["--out", out] + extra, cwd=str(tmp_path), capture_output=True, text=True, timeout=300)
        assert done.returncode == 0, done.stderr[-2000:]
        outs.append(np.load(out, allow_pickle=False))
    assert sorted(os.listdir(index_dir)) == sorted(S._FILES + S._FP8_FILES[:1])
    assert np.load(os.path.join(index_dir, "tokens.npy"), mmap_mode="r").dtype == np.uint8
    a, b = outs
    assert a["ids"].shape == (80, 5) and sorted(a.files) == sorted(b.files)
    for key in a.files:
        assert np.array_equal(a[key], b[key]), key
