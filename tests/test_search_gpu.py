"""Late-interaction search on the GPU: `clipx_topk_merge` (csrc/topk.hip) and `LateInteractionIndex` (colxlip_amd/search.py).

Every comparison of a selection is EXACT equality of values and positions with `search.topk_reference` (stable sorts on the CPU)
on the CPU copy of the same scores: the kernel copies values and the order is total, so there is nothing to tolerate."""
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
from colxlip_amd.data import get_data  # noqa: E402
from colxlip_amd.search import LateInteractionIndex, topk_reference  # noqa: E402
from oracle import clip_oracle as O  # noqa: E402
from tests import late_interaction_ref as R  # noqa: E402
from tests.late_interaction_ref import Q49  # noqa: E402

DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")


def _equal(got, want, what=""):
    gv, gi = got[0].cpu(), got[1].cpu().to(torch.int32)
    assert gv.shape == want[0].shape and gi.shape == want[1].shape, what
    assert torch.equal(gi, want[1]), (what, (gi != want[1]).nonzero()[:4].tolist())
    assert torch.equal(gv.view(torch.int32), want[0].view(torch.int32)), what          # bit for bit


def _tile_in_frame(nq, nc, query_dim, seed):
    """A [nc, nq] (query_dim 1) or [nq, nc] (query_dim 0) view inside a larger buffer of +inf: whatever the kernel reads
    outside the view would win every comparison.  Values from a small set, so ties are everywhere."""
    g = torch.Generator().manual_seed(seed)
    rows, cols = (nc, nq) if query_dim == 1 else (nq, nc)
    frame = torch.full((rows + 3, cols + 5), INF)
    frame[1:1 + rows, 2:2 + cols] = torch.randint(-20, 20, (rows, cols), generator=g).float() / 4
    frame = frame.to(DEV)
    return frame[1:1 + rows, 2:2 + cols]


# ------------------------------------------------------------------------------------------------ 1. the kernel, shape grid
@pytest.mark.parametrize("k", [1, 5, 10, 64, 256])
@pytest.mark.parametrize("query_dim", [1, 0])
def test_kernel_grid(query_dim, k):
    """query_dim 1: lane per query (q_stride 1); query_dim 0: wave per query (c_stride 1).  Sizes around the 64-lane group and
    the kernels' steps (32 rows / 512 candidates), one and several workgroups, k above the candidate count."""
    for nq in (1, 63, 64, 65, 130):
        for nc in (1, 63, 64, 65, 257, 1000):
            view = _tile_in_frame(nq, nc, query_dim, seed=nq * 1000 + nc)
            assert view.stride(1) == 1 and view.stride(0) == view.shape[1] + 5
            best = ops.topk_init(nq, k, DEV)
            ops.topk_merge(view, query_dim, 777, *best)
            want = topk_reference(view.cpu(), k, query_dim, c_base=777)
            _equal(best, want, (nq, nc, k, query_dim))
            if k > nc:
                assert bool((best[1][:, nc:] == -1).all()) and bool((best[0][:, nc:] == -INF).all())
                assert bool((best[1][:, :nc] >= 777).all())


@pytest.mark.parametrize("nq,nc,k", [(16390, 130, 7), (32773, 70, 7), (32773, 70, 256)])
def test_kernel_wide_query_groups(nq, nc, k):
    """Lane per query: up to 16 352 queries a workgroup owns 16 of them (every shape of test_kernel_grid), from 16 353 on 32, from
    32 705 on 64 (512 workgroups before the rows are made wider).  A partial last group and several steps in both; k = 256 is the
    largest list, 145 KiB of LDS at 64 queries."""
    view = _tile_in_frame(nq, nc, 1, seed=nq + k)
    best = ops.topk_init(nq, k, DEV)
    ops.topk_merge(view[:nc // 2], 1, 5, *best)
    ops.topk_merge(view[nc // 2:], 1, 5 + nc // 2, *best)
    _equal(best, topk_reference(view.cpu(), k, 1, c_base=5), (nq, nc, k))


# ------------------------------------------------------------------------------------------------ 2. merging
N_GALLERY = 1000
CUTS = {1: [0, 1000], 3: [0, 333, 401, 1000],
        16: [0, 1, 64, 65, 129, 200, 333, 334, 400, 512, 513, 700, 701, 702, 900, 999, 1000]}


def _gallery(kind, nq):
    g = torch.Generator().manual_seed(11)
    pos = torch.arange(N_GALLERY, dtype=torch.float32)
    if kind == "ascending":                       # every candidate is inserted
        s = (pos / 8).expand(nq, N_GALLERY).clone() + torch.arange(nq, dtype=torch.float32).unsqueeze(1)
    elif kind == "descending":                    # none after the first k
        s = (-pos / 8).expand(nq, N_GALLERY).clone()
    elif kind == "equal":                         # positions 0 .. k-1
        s = torch.full((nq, N_GALLERY), 0.25)
    elif kind == "boundary_duplicates":           # the best value sits on both sides of tile boundaries
        s = torch.randn(nq, N_GALLERY, generator=g)
        for b in (333, 401, 513, 900):
            s[:, b - 1] = s[:, b] = 7.0
        s[::2, 64] = s[::2, 63] = 7.0
    elif kind == "inf_and_nan":
        s = torch.randn(nq, N_GALLERY, generator=g)
        s[torch.rand(nq, N_GALLERY, generator=g) < 0.3] = -INF
        s[torch.rand(nq, N_GALLERY, generator=g) < 0.3] = float("nan")
        s[3, :] = float("nan")                    # a query that takes nothing at all
        s[4, 5:] = -INF                           # ... and one with fewer candidates than k
    return s


@pytest.mark.parametrize("kind", ["ascending", "descending", "equal", "boundary_duplicates", "inf_and_nan"])
@pytest.mark.parametrize("query_dim", [1, 0])
def test_merging_is_independent_of_the_tiling(query_dim, kind):
    nq = 70
    s = _gallery(kind, nq)                                              # [nq, gallery]
    dense = (s.t().contiguous() if query_dim == 1 else s).to(DEV)      # image-major for lane-per-query
    for k in (10, 100):
        want = topk_reference(s, k, 0)
        if kind == "equal":
            assert want[1].tolist() == [list(range(k))] * nq
        for pieces, cuts in CUTS.items():
            tiles = list(zip(cuts[:-1], cuts[1:]))
            shuffled = [tiles[i] for i in torch.randperm(len(tiles), generator=torch.Generator().manual_seed(pieces)).tolist()]
            for order in (tiles, tiles[::-1], shuffled):
                best = ops.topk_init(nq, k, DEV)
                for lo, hi in order:
                    ops.topk_merge(dense[lo:hi] if query_dim == 1 else dense[:, lo:hi], query_dim, lo, *best)
                _equal(best, want, (kind, k, pieces, order[0]))


# ------------------------------------------------------------------------------------------------ 3. refusals
def test_refusals_launch_nothing():
    s = torch.randn(8, 6, device=DEV)
    best = ops.topk_init(8, 4, DEV)
    ops.topk_merge(s, 0, 0, *best)
    before = (best[0].clone(), best[1].clone())
    big = torch.ones(16, 12, device=DEV) * 99
    cases = [
        lambda: ops.topk_merge(big[:8, :6], 0, 0, torch.empty((8, 0), device=DEV), torch.empty((8, 0), dtype=torch.int32, device=DEV)),
        lambda: ops.topk_merge(big[:8, :6], 0, 0, torch.full((8, 257), -INF, device=DEV),
                               torch.full((8, 257), -1, dtype=torch.int32, device=DEV)),
        lambda: ops.topk_merge(big[::2, ::2], 0, 0, *best),                     # both strides different from 1
        lambda: ops.topk_merge(big[:8, :6], 0, 2 ** 31 - 6, *best),             # c_base + nc = 2^31
        lambda: ops.topk_merge(big[:8, :6], 0, -1, *best),
    ]
    for case in cases:
        with pytest.raises(RuntimeError, match="topk_merge"):
            case()
        assert torch.equal(best[0], before[0]) and torch.equal(best[1], before[1])
    ops.topk_merge(big[:8, :0], 0, 0, *best)                                    # no candidates
    ops.topk_merge(big[:0, :6], 0, 0, best[0][:0], best[1][:0])                 # no queries
    ops.topk_merge(big[:0, :8].t(), 0, 0, *best)
    torch.cuda.synchronize()
    assert torch.equal(best[0], before[0]) and torch.equal(best[1], before[1])
    ramp = (100 + torch.arange(6.0)).repeat(8, 1).to(DEV)
    ops.topk_merge(ramp, 0, 2 ** 31 - 7, *best)                                 # the last position int32 holds is accepted
    assert best[1][:, 0].tolist() == [2 ** 31 - 2] * 8 and best[0][:, 0].tolist() == [105.0] * 8


# ------------------------------------------------------------------------------------------------ 4. index vs the dense route
ROUTES = {"fused_bf16": (49, 128, torch.bfloat16, 0.4), "general_fp32": (16, 64, torch.float32, 0.4), "global_only": (49, 128, None, 1.0)}


@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("kind", ["image", "text"])
def test_index_equals_dense_route(kind, route, monkeypatch):
    """35 = 2 * 16 + 3 gallery items in chunks of 16 (the last chunk is neither full nor, at 49 tokens, a multiple of the GEMM's
    8-image alignment unit), queries in chunks too.  The reference: `ops.maxsim_scores` on every (query chunk, gallery chunk) with
    the same boundaries, concatenated into the dense matrix, then `topk_reference`."""
    q, e, dtype, alpha = ROUTES[route]
    scale, n_gal, n_qry = 13.5, 35, 19
    monkeypatch.setattr(LateInteractionIndex, "CHUNK_ITEMS", 16)
    monkeypatch.setattr(LateInteractionIndex, "QUERY_CHUNK", 8)
    n_img, n_txt = (n_gal, n_qry) if kind == "image" else (n_qry, n_gal)
    img_f, txt_f = R.features(n_img, e, 1).to(DEV), R.features(n_txt, e, 2).to(DEV)
    img_t = None if dtype is None else R.image_tokens(n_img, q, e, 3, dtype).to(DEV)
    txt_t = None if dtype is None else R.text_tokens(n_txt, 20, e, 4, dtype).to(DEV)
    gal_f, gal_t, qry_f, qry_t = (img_f, img_t, txt_f, txt_t) if kind == "image" else (txt_f, txt_t, img_f, img_t)
    ids = 1000 + 3 * torch.arange(n_gal)
    routes_taken = []
    fold, reduce_ = ops.maxsim_score_fold, ops.maxsim_reduce
    monkeypatch.setattr(ops, "maxsim_score_fold", lambda *a: (routes_taken.append("fold" if a[8] is not None else "global"), fold(*a))[1])
    monkeypatch.setattr(ops, "maxsim_reduce", lambda *a: (routes_taken.append("general"), reduce_(*a))[1])

    index = LateInteractionIndex(kind, alpha=alpha, scale=scale, device=DEV)
    index.add(gal_f[:20], None if gal_t is None else gal_t[:20], ids=ids[:20])
    index.add(gal_f[20:], None if gal_t is None else gal_t[20:], ids=ids[20:])
    assert [c[1].shape[0] for c in index.chunks()] == [16, 16, 3]
    merges = []
    merge = ops.topk_merge
    monkeypatch.setattr(ops, "topk_merge", lambda s, qd, base, bv, bi: (merges.append((tuple(s.shape), qd, base)), merge(s, qd, base, bv, bi))[1])
    got5 = index.search(qry_f, qry_t, 5)
    n_calls = len(routes_taken)
    got40 = index.search(qry_f, qry_t, 40)
    assert len(routes_taken) == 2 * n_calls and n_calls >= 9
    assert set(routes_taken) == {{"fused_bf16": "fold", "general_fp32": "general", "global_only": "global"}[route]}

    # the dense route over the same boundaries
    dense = torch.empty(n_img, n_txt, device=DEV)
    qchunk = 8                                       # 8 images x 49 or 16 tokens: already aligned
    for q0 in range(0, n_qry, qchunk):
        q1 = min(n_qry, q0 + qchunk)
        for g0 in range(0, n_gal, 16):
            g1 = min(n_gal, g0 + 16)
            (i0, i1, t0, t1) = (g0, g1, q0, q1) if kind == "image" else (q0, q1, g0, g1)
            G = TR.similarity_matrix(img_f[i0:i1], txt_f[t0:t1])
            ops.maxsim_scores(None if img_t is None else img_t[i0:i1], None if txt_t is None else txt_t[t0:t1], G, alpha, scale,
                              out=dense[i0:i1, t0:t1])
    # the merges saw only real items: 16, 16, 3 per query chunk, at bases 0, 16, 32
    per_search = [(m[0][0] if kind == "image" else m[0][1], m[2]) for m in merges[:len(merges) // 2]]
    assert per_search == [(16, 0), (16, 16), (3, 32)] * 3 and all(m[1] == (1 if kind == "image" else 0) for m in merges)
    for got, k in ((got5, 5), (got40, 40)):
        want_v, want_p = topk_reference(dense.cpu(), k, 1 if kind == "image" else 0)
        assert got[0].is_cuda and got[1].is_cuda and got[1].dtype == torch.int64 and got[0].dtype == torch.float32
        want_ids = torch.where(want_p >= 0, ids[want_p.clamp(min=0).long()], torch.full_like(want_p, -1).long())
        assert torch.equal(got[1].cpu(), want_ids), route
        assert torch.equal(got[0].cpu().view(torch.int32), want_v.view(torch.int32)), route
        assert set(got[1].cpu().flatten().tolist()) <= set(ids.tolist()) | {-1}          # no padded item
    assert bool((got40[1][:, 35:] == -1).all()) and bool((got40[1][:, :35] >= 0).all())
    assert bool((got40[0][:, 35:] == -INF).all())


# ------------------------------------------------------------------------------------------------ 5. the reference's numbers
def test_orderings_equal_reference_fixture(golden_dir):
    """tests/golden/late_interaction.npz (6 images, 10 captions; `scores` from the reference's compute_colbert_similarity): the full
    orderings `search` returns are the descending argsort of the stored scores, the reference's own ranking step, for every
    query; the values lie within the 2e-5 the scorer is held to on this fixture (neighbouring sorted scores are at least 0.014
    apart)."""
    z = np.load(os.path.join(golden_dir, "late_interaction.npz"), allow_pickle=False)
    stored = torch.from_numpy(z["scores"])                                           # [6 images, 10 captions]
    fi, ft = torch.from_numpy(z["image_features"]).to(DEV), torch.from_numpy(z["text_features"]).to(DEV)
    ti, tt = torch.from_numpy(z["token_image_features"]).to(DEV), torch.from_numpy(z["token_text_features"]).to(DEV)
    alpha, scale = float(z["alpha"]), float(z["scale"])
    images = LateInteractionIndex("image", alpha=alpha, scale=scale, device=DEV).add(fi, ti)
    val, ids = images.search(ft, tt, 6)                                              # text queries
    order = torch.argsort(stored.t(), dim=1, descending=True)
    assert torch.equal(ids.cpu(), order)
    err_t = float((val.cpu() - stored.t().gather(1, order)).abs().max())
    texts = LateInteractionIndex("text", alpha=alpha, scale=scale, device=DEV).add(ft, tt)
    val, ids = texts.search(fi, ti, 10)                                              # image queries
    order = torch.argsort(stored, dim=1, descending=True)
    assert torch.equal(ids.cpu(), order)
    err_i = float((val.cpu() - stored.gather(1, order)).abs().max())
    print(f"reference fixture: max |returned - stored| = {err_t:.3e} (text queries), {err_i:.3e} (image queries)")
    assert err_t < 2e-5 and err_i < 2e-5, (err_t, err_i)


# ------------------------------------------------------------------------------------------------ 6. through a model
SMALL = O.ClipCfg(embed_dim=64, image_size=64, patch_size=16, vision_width=128, vision_layers=2,
                  context_length=77, vocab_size=1024, text_width=128, text_heads=2, text_layers=2)
TINY = O.ClipCfg(embed_dim=32, image_size=32, patch_size=16, vision_width=64, vision_layers=2,
                 context_length=77, vocab_size=512, text_width=64, text_heads=2, text_layers=2)
MODELS = {"ViT-q49-test-colxlip": (Q49, "bf16"), "ViT-small-test-colxlip": (SMALL, "fp32"), "ViT-tiny-test": (TINY, "fp32")}


def _model(name):
    cfg, precision = MODELS[name]
    return R.build_model(name, R.model_state(cfg, heads="colxlip" in name), precision).eval(), cfg, precision


@pytest.mark.parametrize("name", list(MODELS))
def test_search_through_a_model(name):
    """add_images + search_texts and add_texts + search_images against `topk_reference` of model.get_logits under no_grad: one
    gallery chunk and one query chunk, so the tile IS that matrix."""
    model, cfg, precision = _model(name)
    image, text = O.synthetic_batch(cfg, 9, seed=31)
    image, text = image[:8].to(DEV, dtype=torch.bfloat16 if precision == "bf16" else torch.float32), text.to(DEV)
    with torch.no_grad():
        logits, _ = model.get_logits(image, text)                                    # [8 images, 9 texts]
    assert logits.shape == (8, 9)
    images = LateInteractionIndex.from_model(model, "image")
    assert images.alpha == (1.0 if name == "ViT-tiny-test" else model.alpha) and images.prescale == (name == "ViT-tiny-test")
    images.add_images(model, image)              # one batch, as in get_logits: a tower's output may depend on its batch size
    assert len(images) == 8 and images.has_tokens == (name != "ViT-tiny-test")
    if name == "ViT-q49-test-colxlip":
        assert images.chunks()[0][2].dtype == torch.bfloat16 and images.chunks()[0][2].shape == (8, 49, 128)
    for k in (3, 8):
        _equal(images.search_texts(model, text, k), topk_reference(logits.cpu(), k, 1), (name, "t2i", k))
    texts = LateInteractionIndex.from_model(model, "text").add_texts(model, text)
    for k in (4, 12):
        _equal(texts.search_images(model, image, k), topk_reference(logits.cpu(), k, 0), (name, "i2t", k))
    with pytest.raises(ValueError):
        images.search_images(model, image, 3)
    with pytest.raises(ValueError):
        images.add_texts(model, text)


# ------------------------------------------------------------------------------------------------ 7. save / load
def test_loaded_index_returns_identical_results(tmp_path, monkeypatch):
    monkeypatch.setattr(LateInteractionIndex, "CHUNK_ITEMS", 16)
    monkeypatch.setattr(LateInteractionIndex, "IO_ITEMS", 7)
    index = LateInteractionIndex("image", alpha=0.4, scale=20.0, device=DEV)
    index.add(R.features(35, 128, 1).to(DEV), R.image_tokens(35, 49, 128, 3, torch.bfloat16).to(DEV), ids=torch.arange(35) * 2 + 5)
    qf, qt = R.features(19, 128, 2).to(DEV), R.text_tokens(19, 20, 128, 4, torch.bfloat16).to(DEV)
    first = index.search(qf, qt, 10)
    back = LateInteractionIndex.load(index.save(str(tmp_path / "idx")), device=DEV)
    assert len(back) == 35 and [c[1].shape[0] for c in back.chunks()] == [16, 16, 3] and back.chunks()[0][1].is_cuda
    again = back.search(qf, qt, 10)
    assert torch.equal(first[1], again[1]) and torch.equal(first[0].view(torch.int32), again[0].view(torch.int32))
    assert int(first[1].min()) >= 5


# ------------------------------------------------------------------------------------------------ 8. memory
@pytest.mark.parametrize("route", ["global", "fused"])
def test_peak_memory_does_not_grow_with_the_gallery(route, monkeypatch):
    """512 (global route) / 64 (fused token route) queries, k = 10, gallery chunks of 256 items: what `search` allocates above what
    is live before it is the same, within 64 KiB, for 2 048 and 4 096 gallery items.  The dense matrix of the larger gallery would
    add 4 MiB (global route: 2 048 more items x 512 queries x 4 B)."""
    monkeypatch.setattr(LateInteractionIndex, "CHUNK_ITEMS", 256)
    e = 128
    if route == "global":
        qf, qt = R.features(512, e, 2).to(DEV), None
    else:
        qf, qt = R.features(64, e, 2).to(DEV), R.text_tokens(64, 20, e, 4, torch.bfloat16).to(DEV)
    peaks = []
    for n in (2048, 4096):
        index = LateInteractionIndex("image", alpha=1.0 if route == "global" else 0.5, scale=10.0, device=DEV)
        index.add(R.features(n, e, 1).to(DEV), None if route == "global" else R.image_tokens(n, 16, e, 3, torch.bfloat16).to(DEV))
        index.search(qf, qt, 10)                                   # warm: library handles, kernel attributes
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        live = torch.cuda.memory_allocated()
        val, ids = index.search(qf, qt, 10)
        torch.cuda.synchronize()
        peaks.append(torch.cuda.max_memory_allocated() - live)
        assert int(ids.max()) < n and int(ids.min()) >= 0
        del index, val, ids
    print(f"search peak above live memory ({route}): {peaks[0]} B at 2048 items, {peaks[1]} B at 4096 items")
    assert abs(peaks[1] - peaks[0]) <= 64 * 1024, peaks
    if route == "global":
        assert peaks[1] < 4 * 1024 * 1024, peaks                   # below the dense matrix alone


# ------------------------------------------------------------------------------------------------ 9. command line
@pytest.fixture(scope="module")
def cli_case(tmp_path_factory):
    """ViT-small-test-colxlip (fp32) on a synthetic retrieval split of 64 images x 5 captions: evaluate()'s metrics, the dense
    scores, and a checkpoint the child processes load."""
    name = "ViT-small-test-colxlip"
    model, cfg, precision = _model(name)
    tmp = tmp_path_factory.mktemp("search_cli")
    ckpt = str(tmp / "model.pt")
    torch.save({"state_dict": {k: v.detach().cpu() for k, v in model.state_dict().items()}}, ckpt)
    argv = ["--model", name, "--dataset-type", "synthetic", "--precision", precision, "--batch-size", "16", "--retrieval-coco",
            "--val-num-samples", "64", "--alpha", "0.5"]
    args = S.parse_args(argv)
    args.rank, args.local_rank, args.world_size, args.distributed, args.device = 0, 0, 1, False, "cuda"
    args.save_logs, args.wandb = False, False
    data = get_data(args, model=model)
    metrics = TR.evaluate(model, data, 1, args)
    txt, img, img2txt, txt2img = data["retrieval_coco"]
    dense, img_ids, cap_ids = TR.late_interaction_scores(model, txt.dataloader, img.dataloader, torch.device("cuda"), torch.float32, 0.5)
    return dict(argv=argv, ckpt=ckpt, tmp=tmp, metrics=metrics, dense=dense.cpu(), img_ids=img_ids, cap_ids=cap_ids,
                img2txt=img2txt, txt2img=txt2img)


@pytest.mark.parametrize("direction", ["t2i", "i2t"])
def test_cli_recalls_equal_evaluate(cli_case, direction):
    c = cli_case
    dense = c["dense"] if direction == "i2t" else c["dense"].t()                     # [queries, gallery]
    assert dense.shape == ((64, 320) if direction == "i2t" else (320, 64))
    top = torch.sort(dense, dim=1, descending=True)[0]
    for K in (1, 5, 10):                             # the equality of the recalls below rests on this
        assert bool((top[:, K - 1] > top[:, K]).all()), f"an exact tie straddles rank {K}: R@{K} is ambiguous"
    out = str(c["tmp"] / f"{direction}.npz")
    index_dir = str(c["tmp"] / f"index_{direction}")
    cmd = [sys.executable, *(["-s"] if sys.flags.no_user_site else []), "-c", R.LAUNCHER, ROOT, *c["argv"], "--pretrained", c["ckpt"],
           "--direction", direction, "--k", "10", "--out", out, "--save-index", index_dir]
    done = subprocess.run(cmd, cwd=str(c["tmp"]), capture_output=True, text=True, timeout=300)
    assert done.returncode == 0, done.stderr[-2000:]
    assert "Search retrieval_coco " + direction in done.stderr
    z = np.load(out, allow_pickle=False)
    assert z["scores"].shape == z["ids"].shape == (dense.shape[0], 10) and z["ids"].dtype == np.int64
    query_ids, gallery_ids = (c["cap_ids"], c["img_ids"]) if direction == "t2i" else (c["img_ids"], c["cap_ids"])
    assert z["query_ids"].tolist() == query_ids.tolist()
    assert bool((z["scores"][:, :-1] >= z["scores"][:, 1:]).all()) and set(z["ids"].flatten().tolist()) <= set(gallery_ids.tolist())
    truth = c["txt2img"] if direction == "t2i" else c["img2txt"]
    name = "text_to_image" if direction == "t2i" else "image_to_text"
    got = S.recall_at(z["ids"], z["query_ids"], truth)
    reported = dict(zip(z["metric_names"].tolist(), z["metric_values"].tolist()))
    for K in (1, 5, 10):
        assert got[K] == c["metrics"][f"retrieval_coco_{name}_R@{K}"] == reported[f"{name}_R@{K}"], (K, got, reported)
    assert sorted(os.listdir(index_dir)) == sorted(S._FILES)
