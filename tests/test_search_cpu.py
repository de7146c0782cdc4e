"""Late-interaction search, the parts that need no GPU: the torch reference selection against a brute-force Python one, index
storage and its files, the chunk plan, the command line, and the new C-ABI entry's prototype."""
import ctypes
import json
import math
import os

import numpy as np
import pytest
import torch

import colxlip_amd
from colxlip_amd import _lib, ops
from colxlip_amd import search as S
from colxlip_amd.search import LateInteractionIndex, topk_reference


def _brute(rows, k, c_base=0, old=None):
    """rows: list (one per query) of candidate value lists -> ([values], [positions]) per query by a Python sort"""
    vals, poss = [], []
    for j, row in enumerate(rows):
        cand = [(v, c_base + c) for c, v in enumerate(row) if not math.isnan(v) and v != float("-inf")]
        if old is not None:
            cand += [(v, p) for v, p in zip(old[0][j].tolist(), old[1][j].tolist()) if p >= 0]
        cand.sort(key=lambda t: (-t[0], t[1]))
        cand = cand[:k] + [(float("-inf"), -1)] * max(0, k - len(cand))
        vals.append([v for v, _ in cand])
        poss.append([p for _, p in cand])
    return torch.tensor(vals, dtype=torch.float32), torch.tensor(poss, dtype=torch.int32)


def _same(got, want):
    assert got[0].dtype == torch.float32 and got[1].dtype == torch.int32
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


@pytest.mark.parametrize("k", [1, 3, 7, 40])
def test_topk_reference_vs_brute_force(k):
    g = torch.Generator().manual_seed(k)
    s = torch.randint(0, 6, (9, 23), generator=g).float()                  # few distinct values: ties everywhere
    s[2, 5] = float("nan")
    s[3, :] = float("-inf")
    s[4, 1] = float("-inf")
    s[5, 0] = float("inf")
    _same(topk_reference(s, k, 0, c_base=100), _brute(s.tolist(), k, 100))
    _same(topk_reference(s.t().contiguous(), k, 1, c_base=100), _brute(s.tolist(), k, 100))
    assert k <= 23 or bool((topk_reference(s, k, 0)[1][:, 23:] == -1).all())


def test_topk_reference_split_and_merge():
    g = torch.Generator().manual_seed(0)
    s = torch.randint(0, 4, (5, 50), generator=g).float()
    for k in (4, 60):
        whole = topk_reference(s, k, 0)
        for cuts in ([0, 50], [0, 7, 8, 31, 50], [0, 25, 50]):
            tiles = list(zip(cuts[:-1], cuts[1:]))
            for order in (tiles, tiles[::-1]):
                best = None
                for lo, hi in order:
                    best = topk_reference(s[:, lo:hi], k, 0, c_base=lo, best=best)
                _same(best, whole)
        _same(whole, _brute(s.tolist(), k))
    old = topk_reference(s[:, :10], 4, 0)
    _same(topk_reference(s[:, 10:], 4, 0, c_base=10, best=old), _brute(s[:, 10:].tolist(), 4, 10, old=old))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("kind", ["image", "text"])
def test_index_add_save_load_round_trip(tmp_path, monkeypatch, dtype, kind):
    monkeypatch.setattr(LateInteractionIndex, "CHUNK_ITEMS", 8)
    monkeypatch.setattr(LateInteractionIndex, "IO_ITEMS", 5)
    g = torch.Generator().manual_seed(1)
    feats = torch.randn(21, 32, generator=g)
    toks = torch.randn(21, 6, 32, generator=g).to(dtype)
    ids = torch.randperm(1000, generator=g)[:21].to(torch.int64)
    index = LateInteractionIndex(kind, alpha=0.3, scale=17.5, device="cpu")
    for lo, hi in ((0, 3), (3, 16), (16, 21)):                                # adds that end inside, at and across chunk ends
        index.add(feats[lo:hi], toks[lo:hi], ids=ids[lo:hi])
    assert len(index) == 21 and [c[1].shape[0] for c in index.chunks()] == [8, 8, 5]
    assert [c[0] for c in index.chunks()] == [0, 8, 16]
    assert torch.equal(torch.cat([c[1] for c in index.chunks()]), feats)
    assert torch.equal(torch.cat([c[2] for c in index.chunks()]).view(torch.int16 if dtype == torch.bfloat16 else dtype),
                       toks.view(torch.int16 if dtype == torch.bfloat16 else dtype))
    path = index.save(str(tmp_path / "idx"))
    assert sorted(os.listdir(path)) == sorted(S._FILES)
    with open(os.path.join(path, "meta.json")) as f:
        meta = json.load(f)
    assert meta["kind"] == kind and meta["alpha"] == 0.3 and meta["scale"] == 17.5 and meta["n"] == 21
    assert meta["tokens"] == [6, 32] and meta["token_dtype"] == ("bfloat16" if dtype == torch.bfloat16 else "float32")
    stored = np.load(os.path.join(path, "tokens.npy"))
    assert stored.dtype == (np.uint16 if dtype == torch.bfloat16 else np.float32) and stored.shape == (21, 6, 32)
    back = LateInteractionIndex.load(path, device="cpu")
    assert (back.kind, back.alpha, back.scale, len(back)) == (kind, 0.3, 17.5, 21)
    assert torch.equal(back.ids, ids) and not back._running_ids
    assert torch.equal(torch.cat([c[1] for c in back.chunks()]), feats)
    got = torch.cat([c[2] for c in back.chunks()])
    assert got.dtype == dtype and torch.equal(got.view(torch.int16 if dtype == torch.bfloat16 else dtype),
                                              toks.view(torch.int16 if dtype == torch.bfloat16 else dtype))


def test_index_without_tokens_and_refusals(tmp_path):
    feats = torch.randn(5, 16)
    index = LateInteractionIndex("image", alpha=1.0, scale=2.0, device="cpu")
    index.add(feats[:2]).add(feats[2:])
    assert not index.has_tokens and index.ids.tolist() == [0, 1, 2, 3, 4] and index._running_ids
    path = index.save(str(tmp_path / "idx"))
    assert "tokens.npy" not in os.listdir(path)
    back = LateInteractionIndex.load(path, device="cpu")
    assert back._running_ids and torch.equal(back.chunks()[0][1], feats) and not back.has_tokens
    with pytest.raises(ValueError, match="alpha"):
        LateInteractionIndex("image", alpha=0.5, device="cpu").add(feats)
    with pytest.raises(ValueError, match="kind"):
        LateInteractionIndex("audio", device="cpu")
    with pytest.raises(ValueError, match="prescale"):
        LateInteractionIndex("image", alpha=0.5, prescale=True, device="cpu")
    with pytest.raises(ValueError, match="fp32"):
        LateInteractionIndex("image", alpha=1.0, device="cpu").add(feats.double())
    assert colxlip_amd.LateInteractionIndex is LateInteractionIndex


@pytest.mark.parametrize("q", [16, 49, 196])
def test_chunk_plan_respects_gemm_alignment(monkeypatch, q):
    for limit in (1, 3, 16, 100, 16384, 10 ** 6):
        ci = S.image_chunk_items(limit, q)
        assert ci >= 1 and (ci * q) % 8 == 0 and ci <= ops.MAXSIM_MAX_IMAGES
        unit = 8 // math.gcd(q, 8)
        assert ci <= max(limit, unit) and ci + unit > min(limit, ops.MAXSIM_MAX_IMAGES)      # the largest such count
        monkeypatch.setattr(LateInteractionIndex, "CHUNK_ITEMS", limit)
        index = LateInteractionIndex("image", alpha=0.5, device="cpu")
        index.add(torch.zeros(1, 8), torch.zeros(1, q, 8))
        assert index._chunk == ci
        texts = LateInteractionIndex("text", alpha=0.5, device="cpu")        # a text gallery has no alignment to keep
        texts.add(torch.zeros(1, 8), torch.zeros(1, q, 8))
        assert texts._chunk == limit


def test_cli_arguments():
    a = S.parse_args(["--model", "ViT-B-32-colxlip", "--precision", "bf16", "--dataset-type", "packed", "--val-data", "/d",
                      "--retrieval-coco", "--direction", "i2t", "--k", "25", "--out", "r.npz", "--save-index", "idx"])
    assert (a.model, a.precision, a.dataset_type, a.val_data, a.retrieval_coco) == ("ViT-B-32-colxlip", "bf16", "packed", "/d", True)
    assert (a.direction, a.k, a.out, a.save_index, a.load_index) == ("i2t", 25, "r.npz", "idx", None)
    d = S.parse_args(["--model", "ViT-B-32", "--dataset-type", "synthetic", "--retrieval-coco"])
    assert (d.direction, d.k, d.out, d.save_index, d.load_index, d.pretrained) == ("t2i", 10, None, None, None, "")
    for bad in (["--k", "0"], ["--k", "257"], ["--direction", "x2y"], ["--save-index", "a", "--load-index", "b"]):
        with pytest.raises(SystemExit):
            S.parse_args(["--model", "ViT-B-32", *bad])


def test_recall_at():
    ids = np.array([[5, 7, 9], [1, 2, 3], [4, 4, 4]])
    got = S.recall_at(ids, [10, 11, 12], {10: [9], 11: 1, 12: [8, 6]}, ks=(1, 3, 10))
    assert got == {1: 1 / 3, 3: 2 / 3}


def test_topk_entry_prototype_and_cpu_refusal():
    protos = {name: (res, args) for name, res, args in _lib.header_prototypes()}
    res, args = protos["clipx_topk_merge"]
    assert res is ctypes.c_int
    assert args == [ctypes.c_int] * 3 + [ctypes.c_void_p] + [ctypes.c_long] * 3 + [ctypes.c_void_p] * 3
    assert hasattr(ctypes.CDLL(_lib.lib_path()), "clipx_topk_merge")
    with pytest.raises(RuntimeError, match="no CPU"):
        ops.topk_merge(torch.zeros(4, 4), 0, 0, torch.zeros(4, 2), torch.zeros(4, 2, dtype=torch.int32))
    with pytest.raises(ValueError):
        ops.topk_init(4, 0, "cpu")
    with pytest.raises(ValueError):
        ops.topk_init(4, 257, "cpu")
    v, i = ops.topk_init(3, 5, "cpu")
    assert v.shape == (3, 5) and bool((v == float("-inf")).all()) and i.dtype == torch.int32 and bool((i == -1).all())
    # the refusals of the entry itself need no device: they come before any launch
    fn = _lib.lib().clipx_topk_merge
    for nq, nc, k, qs, cs, base in ((4, 4, 0, 1, 4, 0), (4, 4, 257, 1, 4, 0), (4, 4, 2, 2, 8, 0), (4, 4, 2, 1, 4, 2 ** 31 - 4),
                                    (4, 4, 2, 1, 4, -1)):
        assert fn(nq, nc, k, None, qs, cs, base, None, None, None) != 0
        assert b"topk_merge" in _lib.lib().clipx_last_error()
    assert fn(0, 4, 2, None, 1, 4, 0, None, None, None) == 0 and fn(4, 0, 2, None, 1, 4, 0, None, None, None) == 0
