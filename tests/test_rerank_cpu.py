"""Reranking (`LateInteractionIndex.rerank`, `search(candidates=C)`, `ops.maxsim_pair_scores`, csrc/maxsim_pairs.hip): what needs no
device -- the command line, the C prototype and the refusals its entry makes before it touches the device, the shape predicate,
the count-to-weight rule, and the index's refusals."""
import ctypes

import pytest
import torch

from colxlip_amd import _lib, ops
from colxlip_amd import search as S
from colxlip_amd.search import LateInteractionIndex
from tests.late_interaction_ref import counts_model, einsum_ref, image_tokens, text_tokens


def test_cli_candidates():
    base = ["--model", "ViT-B-32-colxlip", "--dataset-type", "synthetic", "--retrieval-coco"]
    assert S.parse_args(base).candidates == 0                                       # exhaustive
    a = S.parse_args(base + ["--k", "10", "--candidates", "64"])
    assert (a.k, a.candidates) == (10, 64)
    assert S.parse_args(base + ["--k", "10", "--candidates", "10"]).candidates == 10
    assert S.parse_args(base + ["--k", "256", "--candidates", "256"]).candidates == 256
    for bad in (["--k", "10", "--candidates", "9"], ["--candidates", "257"], ["--candidates", "-1"],
                ["--candidates", "64", "--index-dtype", "fp8"], ["--candidates", "64", "--evaluate-as-original-clip"]):
        with pytest.raises(SystemExit):
            S.parse_args(base + bad)


def test_pairs_prototype_and_entry_refusals():
    protos = {name: (res, args) for name, res, args in _lib.header_prototypes()}
    res, args = protos["clipx_maxsim_pairs"]
    V, I, L, F = ctypes.c_void_p, ctypes.c_int, ctypes.c_long, ctypes.c_float
    assert res is I
    assert args == [I] * 6 + [V] * 4 + [I, I, L, V, L, V, L, V, L, F, F, F, V, V]
    assert hasattr(ctypes.CDLL(_lib.lib_path()), "clipx_maxsim_pairs")
    fn = _lib.lib().clipx_maxsim_pairs

    def call(gi=1, nq=4, C=8, q=49, n=77, e=128, n_chunks=3, chunk=16, items=35, cand_stride=8, ld_gp=8, ld_out=8):
        return fn(gi, nq, C, q, n, e, None, None, None, None, n_chunks, chunk, items, None, cand_stride, None, ld_gp, None, ld_out,
                  0.5, 0.5, 1.0, None, None)

    # every one of these is refused on the arguments alone: no pointer is looked at, nothing is launched
    for kw in (dict(q=15), dict(e=64), dict(e=160), dict(n=81), dict(gi=0, q=81), dict(gi=0, q=80, e=1024), dict(cand_stride=9),
               dict(ld_out=7), dict(items=49), dict(chunk=0), dict(nq=-1), dict(C=8 * 65535 + 1, cand_stride=8 * 65535 + 1)):
        assert call(**kw) != 0, kw
        assert b"maxsim_pairs" in _lib.lib().clipx_last_error(), kw
    assert call(gi=0, q=80, n=500) == -1 and b"null pointer" in _lib.lib().clipx_last_error()       # a shape it takes: the next check
    assert call(nq=0) == 0 and call(C=0, cand_stride=0, ld_out=0, ld_gp=0) == 0                      # nothing to do


def test_shape_predicate():
    T = ops.maxsim_pairs_takes
    assert T(49, 77, 512) and T(16, 20, 128) and T(80, 80, 512) and T(64, 77, 768)
    assert not T(15, 77, 512) and not T(49, 77, 64) and not T(49, 77, 160) and not T(49, 77, 96)
    # the staged side: the text over an image gallery, the image over a text gallery
    assert T(196, 77, 512, gallery_is_image=True) and not T(196, 77, 512, gallery_is_image=False) and not T(196, 77, 512)
    assert T(49, 300, 512, gallery_is_image=False) and not T(49, 300, 512, gallery_is_image=True)
    assert T(80, 77, 768) and not T(80, 77, 1024, gallery_is_image=False)          # 80 x 1032 x 2 bytes > 128 KiB
    assert T(64, 77, 1016 // 64 * 64, gallery_is_image=False)


def test_count_to_weight_rule():
    """The kernel's text side in plain torch: the first cnt rows, the last of them weighted n - cnt + 1, divided by n -- against
    the reference's mean over all n rows (`einsum_ref`) on EOT-shaped texts, in fp64 on the bf16 values."""
    q, n, e = 49, 20, 128
    ti = image_tokens(6, q, e, 3).double()
    tt16 = text_tokens(9, n, e, 4)
    tt16[2] = torch.nn.functional.normalize(torch.randn(n, e, generator=torch.Generator().manual_seed(1)), dim=-1).bfloat16()   # no tail
    cnt = counts_model(tt16)
    assert cnt.tolist() == [3, 8, 20, 18, 5, 10, 15, 20, 7]
    tt = tt16.double()
    want = einsum_ref(ti, tt)                                                       # [nt, ni]
    got = torch.empty_like(want)
    for m in range(tt.shape[0]):
        c = int(cnt[m])
        mx = torch.einsum("nd,kqd->knq", tt[m, :c], ti).max(dim=2)[0]              # [ni, c]
        w = torch.ones(c, dtype=torch.float64)
        w[c - 1] = n - c + 1
        got[m] = (mx * w).sum(1) / (n + 1e-8)          # the reference's denominator; in the kernel's fp32 it rounds to n
    assert float((got - want).abs().max()) < 1e-12


def _index(kind, **kw):
    index = LateInteractionIndex(kind, alpha=kw.pop("alpha", 0.4), scale=13.5, device="cpu", **kw)
    tok = None if index.alpha == 1.0 else (image_tokens(5, 16, 64, 3, torch.float32) if kind == "image" else text_tokens(5, 20, 64, 4, torch.float32))
    return index.add(torch.nn.functional.normalize(torch.randn(5, 64), dim=-1), tok)


def test_index_refusals_without_a_device(monkeypatch):
    qf, qt = torch.randn(3, 64), text_tokens(3, 20, 64, 5, torch.float32)
    pos = torch.tensor([[0, 1], [2, -1], [4, 4]])
    index = _index("image")
    for C, k in ((4, 5), (257, 5), (300, 300)):
        with pytest.raises(ValueError, match="candidates"):
            index.search(qf, qt, k, candidates=C)
    with pytest.raises(ValueError, match="outside"):
        index.rerank(qf, qt, torch.tensor([[0, 1], [2, 5], [4, 4]]))                # 5 == len(index)
    with pytest.raises(ValueError, match="outside"):
        index.rerank(qf, qt, torch.tensor([[0, 1], [2, -2], [4, 4]]))
    with pytest.raises(ValueError, match="contiguous"):
        index.rerank(qf, qt, torch.zeros(3, 4, dtype=torch.int64)[:, ::2])
    with pytest.raises(ValueError, match="int32 or int64"):
        index.rerank(qf, qt, pos.float())
    with pytest.raises(ValueError, match="k must be"):
        index.rerank(qf, qt, pos, k=257)
    with pytest.raises(ValueError, match="token features"):
        index.rerank(qf, None, pos)
    for bad in (_index("image", alpha=1.0), _index("image", alpha=1.0, prescale=True)):
        with pytest.raises(ValueError, match="alpha = 1"):
            bad.search(qf, None, 2, candidates=4)
        with pytest.raises(ValueError, match="alpha = 1"):
            bad.rerank(qf, qt, pos)
    monkeypatch.setattr(LateInteractionIndex, "_quantise", lambda self, tokens, n: (tokens.to(torch.uint8), torch.zeros(tokens.shape[:2], dtype=torch.int32)))
    fp8 = LateInteractionIndex("image", alpha=0.4, device="cpu", token_dtype="fp8").add(torch.randn(5, 64), torch.zeros(5, 16, 64))
    with pytest.raises(ValueError, match="fp8"):
        fp8.search(qf, qt, 2, candidates=4)
    with pytest.raises(ValueError, match="fp8"):
        fp8.rerank(qf, qt, pos)
    # candidates=None and 0 are the exhaustive search: on the CPU that reaches the scorer, which has no CPU path
    with pytest.raises(RuntimeError, match="no CPU|device"):
        index.search(qf, qt, 2, candidates=0)


def test_pair_scores_argument_checks():
    cand = torch.zeros(3, 4, dtype=torch.int64)
    tok = torch.zeros(5, 16, 64)
    with pytest.raises(ValueError, match="contiguous"):
        ops.maxsim_pair_scores(torch.zeros(3, 20, 64), [tok], 16, torch.zeros(3, 8, dtype=torch.int64)[:, ::2], None, 0.5, 1.0, True)
    with pytest.raises(ValueError, match="contiguous"):
        ops.maxsim_pair_scores(torch.zeros(3, 20, 64), [tok], 16, torch.zeros(6, 4, dtype=torch.int64)[::2], None, 0.5, 1.0, True)
    with pytest.raises(ValueError, match="Gp"):
        ops.maxsim_pair_scores(torch.zeros(3, 20, 64), [tok], 16, cand, torch.zeros(3, 5), 0.5, 1.0, True)
    with pytest.raises(ValueError, match="needs Gp"):
        ops.maxsim_pair_scores(None, [tok], 16, cand, None, 1.0, 1.0, True)
    with pytest.raises(ValueError, match="chunk_items"):
        ops.maxsim_pair_scores(torch.zeros(3, 20, 64), [tok, tok], 16, cand, None, 0.5, 1.0, True)      # a first chunk of 5 < 16 items
    with pytest.raises(ValueError, match="outside"):
        ops.maxsim_pair_scores(torch.zeros(3, 20, 64), [tok], 16, cand + 5, None, 0.5, 1.0, True)
