"""Reranking on the GPU: `clipx_maxsim_pairs` (csrc/maxsim_pairs.hip) through `ops.maxsim_pair_scores`, `LateInteractionIndex.rerank`
and `search(candidates=C)`.

Scores are held to |score - fp64 reference| <= scale * 2e-5, the bound of the bf16 fused route in test_late_interaction_gpu.py; the
reference is the einsum of the reference's compute_colbert_similarity (`einsum_ref`) in fp64 on the same token values.  Selections
are compared EXACTLY (values bit for bit, ids equal) with `search.topk_reference` on the scores the index itself returned, never
with an ordering of the reference: neighbouring scores of random features lie closer than the bound."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from colxlip_amd import _lib, ops  # noqa: E402
from colxlip_amd import search as S  # noqa: E402
from colxlip_amd import train as TR  # noqa: E402
from colxlip_amd.data import get_data  # noqa: E402
from colxlip_amd.search import LateInteractionIndex, topk_reference  # noqa: E402
from tests import late_interaction_ref as R  # noqa: E402
from tests.late_interaction_ref import Q49  # noqa: E402

DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")
BOUND = 2e-5
N_GAL, CHUNK = 35, 16                       # 16 + 16 + 3: the last chunk is partly filled


def _bits(t):
    return t.contiguous().view(torch.int32)


@functools.lru_cache(maxsize=None)
def _sides(q, n, e, n_img, n_txt, dtype=torch.bfloat16):
    """(image tokens, text tokens, tok [n_txt, n_img] fp64 = MaxSim of every pair) on the CPU; never modified.  The texts are
    EOT-shaped (cnt = 3 .. n) and text 2 keeps distinct rows to the end (cnt = n)."""
    ti, tt = R.image_tokens(n_img, q, e, 3, dtype), R.text_tokens(n_txt, n, e, 4, dtype)
    g = torch.Generator().manual_seed(9)
    tt[2] = torch.nn.functional.normalize(torch.randn(n, e, generator=g), dim=-1).to(dtype)
    return ti, tt, R.einsum_ref(ti.double(), tt.double())


def _candidates(nq, C, seed, n_items=N_GAL):
    """[nq, C] int64: random positions over all chunks, the last item of the last chunk, a duplicate and empty slots"""
    g = torch.Generator().manual_seed(seed)
    cand = torch.randint(0, n_items, (nq, C), generator=g)
    cand[0, 0] = n_items - 1
    if C >= 2:
        cand[:, 1] = cand[:, 0]                                   # a duplicate in every row
    if C >= 3:
        cand[torch.rand(nq, C, generator=g) < 0.2] = -1
        cand[-1, 2] = -1
        cand[0, 0] = n_items - 1
    return cand


def _chunks(t):
    return [t[lo:lo + CHUNK] for lo in range(0, t.shape[0], CHUNK)]


def _pair_reference(tok, cand, gallery_is_image, Gp=None, alpha=0.0, scale=1.0):
    m = (tok if gallery_is_image else tok.t())[:cand.shape[0]].gather(1, cand.clamp(min=0))
    ref = (1.0 - alpha) * m
    if Gp is not None:
        ref = alpha * Gp.double() + ref
    ref = scale * ref
    ref[cand < 0] = -INF
    return ref


def _check(got, ref, cand, bound, what):
    got = got.cpu().double()
    live = cand >= 0
    assert bool((got[~live] == -INF).all()), what
    err = float((got[live] - ref[live]).abs().max()) if bool(live.any()) else 0.0
    assert bool(torch.isfinite(got[live]).all()), what
    return err


# ------------------------------------------------------------------------------------------------ 1. the kernel, shape grid
GRID = [(q, 20, 128) for q in (16, 49, 64, 80)] + [(49, 20, 256), (49, 77, 128)]


@pytest.mark.parametrize("q,n,e", GRID)
@pytest.mark.parametrize("gallery_is_image", [True, False])
def test_kernel_grid(gallery_is_image, q, n, e, monkeypatch):
    """alpha = 0, scale = 1, no global term.  q = 16 .. 80: one to five row tiles, 49 the partial one; E = 128: two 64-element
    k-steps (E = 256: one full 256-element unit); n = 20: texts of 3 .. 20 packed rows (one and two tiles), n = 77: up to five.
    35 gallery items in chunks of 16; C = 1, 7, 64 (less than, and several times, the workgroup's eight waves); 1, 5, 33 queries."""
    assert ops.maxsim_pairs_takes(q, n, e, gallery_is_image)
    n_img, n_txt = (N_GAL, 33) if gallery_is_image else (33, N_GAL)
    ti, tt, tok = _sides(q, n, e, n_img, n_txt)
    gal, qry = (ti, tt) if gallery_is_image else (tt, ti)
    gal_dev, qry_dev = gal.to(DEV), qry.to(DEV)
    chunks = _chunks(gal_dev)
    assert [c.shape[0] for c in chunks] == [16, 16, 3]
    calls = []
    real = _lib.lib().clipx_maxsim_pairs
    monkeypatch.setattr(_lib.lib(), "clipx_maxsim_pairs", lambda *a: (calls.append(a[1:3]), real(*a))[1])
    worst = 0.0
    for nq in (1, 5, 33):
        for C in (1, 7, 64):
            cand = _candidates(nq, C, seed=100 * nq + C)
            got = ops.maxsim_pair_scores(qry_dev[:nq], chunks, CHUNK, cand.to(DEV), None, 0.0, 1.0, gallery_is_image)
            assert got.shape == (nq, C) and got.dtype == torch.float32
            err = _check(got, _pair_reference(tok, cand, gallery_is_image), cand, BOUND, (nq, C))
            worst = max(worst, err)
            assert err <= BOUND, (nq, C, err)
    assert calls == [(nq, C) for nq in (1, 5, 33) for C in (1, 7, 64)]
    print(f"maxsim_pairs {'image' if gallery_is_image else 'text'} gallery q={q} n={n} e={e}: max |score - fp64| = {worst:.3e}")


# ------------------------------------------------------------------------------------------------ 2. masking and frames
@pytest.mark.parametrize("gallery_is_image", [True, False])
def test_masked_rows_and_frames(gallery_is_image):
    """Every similarity of every pair is negative (all tokens lie near +v on the text side and near -v on the image side), so a
    zero padding row of the 49 -> 64 image rows would win the maximum and a padded text row with weight would pull the mean
    towards 0.  `out` and Gp are views inside frames of +inf, the candidate table lies between rows of out-of-range positions:
    what is read or written outside the views shows."""
    q, n, e, nq, C = 49, 20, 128, 9, 11
    g = torch.Generator().manual_seed(5)
    v = torch.nn.functional.normalize(torch.randn(e, generator=g), dim=-1)
    n_img, n_txt = (N_GAL, nq) if gallery_is_image else (nq, N_GAL)
    ti = torch.nn.functional.normalize(-v + 0.03 * torch.randn(n_img, q, e, generator=g), dim=-1).bfloat16()
    tt = torch.nn.functional.normalize(v + 0.03 * torch.randn(n_txt, n, e, generator=g), dim=-1)
    for m in range(n_txt):
        eot = 2 + (5 * m) % (n - 2)
        tt[m, eot:] = tt[m, eot]
    tt = tt.bfloat16()
    tok = R.einsum_ref(ti.double(), tt.double())
    assert float(torch.einsum("mnd,kqd->mknq", tt.double(), ti.double()).max()) < -0.5
    gal, qry = (ti, tt) if gallery_is_image else (tt, ti)
    cand = _candidates(nq, C, seed=3)
    table = torch.full((nq + 2, C), 2 ** 30, dtype=torch.int32)
    table[1:1 + nq] = cand.int()
    table = table.to(DEV)
    frame = torch.full((nq + 3, C + 5), INF, device=DEV)
    gframe = torch.full((nq + 3, C + 5), INF, device=DEV)
    Gp = torch.randn(nq, C, generator=g)
    gframe[1:1 + nq, 2:2 + C] = Gp.to(DEV)
    view, gview = frame[1:1 + nq, 2:2 + C], gframe[1:1 + nq, 2:2 + C]
    assert view.stride(0) == C + 5 and table[1:1 + nq].is_contiguous()
    out = ops.maxsim_pair_scores(qry.to(DEV), _chunks(gal.to(DEV)), CHUNK, table[1:1 + nq], gview, 0.4, 13.5, gallery_is_image, out=view)
    assert out.data_ptr() == view.data_ptr()
    ref = _pair_reference(tok, cand, gallery_is_image, Gp, 0.4, 13.5)
    err = _check(view, ref, cand, 13.5 * BOUND, "masking")
    print(f"maxsim_pairs masking ({'image' if gallery_is_image else 'text'} gallery): max |score - fp64| = {err:.3e} at scale 13.5")
    assert err <= 13.5 * BOUND, err
    outside = torch.ones_like(frame, dtype=torch.bool)
    outside[1:1 + nq, 2:2 + C] = False
    assert bool((frame[outside] == INF).all())


# ------------------------------------------------------------------------------------------------ 3. routes
def _spy(monkeypatch):
    calls = []
    real = _lib.lib().clipx_maxsim_pairs
    monkeypatch.setattr(_lib.lib(), "clipx_maxsim_pairs", lambda *a: (calls.append(a[1:3]), real(*a))[1])
    return calls


@pytest.mark.parametrize("gallery_is_image", [True, False])
@pytest.mark.parametrize("route", ["kernel", "fp32", "e64", "env"])
def test_routes(route, gallery_is_image, monkeypatch):
    q, n = 49, 20
    e = 64 if route == "e64" else 128
    dtype = torch.float32 if route == "fp32" else torch.bfloat16
    if route == "env":
        monkeypatch.setenv("CLIPX_MAXSIM_FUSED", "0")
    n_img, n_txt = (N_GAL, 33) if gallery_is_image else (33, N_GAL)
    ti, tt, tok = _sides(q, n, e, n_img, n_txt, dtype)
    gal, qry = (ti, tt) if gallery_is_image else (tt, ti)
    nq, C = 7, 9
    cand = _candidates(nq, C, seed=17)
    Gp = torch.randn(nq, C, generator=torch.Generator().manual_seed(1))
    calls = _spy(monkeypatch)
    got = ops.maxsim_pair_scores(qry[:nq].to(DEV), _chunks(gal.to(DEV)), CHUNK, cand.to(DEV), Gp.to(DEV), 0.4, 13.5, gallery_is_image)
    assert calls == ([(nq, C)] if route == "kernel" else [])
    err = _check(got, _pair_reference(tok, cand, gallery_is_image, Gp, 0.4, 13.5), cand, 13.5 * BOUND, route)
    assert err <= 13.5 * BOUND, (route, err)
    if route != "kernel":                            # the fallback against the same arithmetic in fp32
        tok32 = R.einsum_ref(ti.float(), tt.float()).double()
        err32 = _check(got, _pair_reference(tok32, cand, gallery_is_image, Gp, 0.4, 13.5), cand, 13.5 * BOUND, route)
        assert err32 <= 13.5 * BOUND, (route, err32)
    print(f"maxsim_pair_scores route {route} ({'image' if gallery_is_image else 'text'} gallery): max |score - fp64| = {err:.3e}")


def test_alpha_one_is_the_global_term(monkeypatch):
    calls = _spy(monkeypatch)
    monkeypatch.setattr(ops, "maxsim_text_counts", lambda *a: pytest.fail("a token kernel ran"))
    Gp = torch.randn(5, 6, device=DEV)
    cand = torch.randint(0, N_GAL, (5, 6), device=DEV)
    got = ops.maxsim_pair_scores(None, [], CHUNK, cand, Gp, 1.0, 13.5, True)
    assert calls == [] and torch.equal(_bits(got), _bits(13.5 * Gp))


# ------------------------------------------------------------------------------------------------ 4. rerank
ROUTES = {"fused_bf16": (49, 128, torch.bfloat16, 0.4), "general_fp32": (16, 64, torch.float32, 0.4)}
SCALE, N_QRY = 13.5, 19


@functools.lru_cache(maxsize=None)
def _case(kind, route):
    """features and tokens of both sides on the CPU and the dense fp64 scores [queries, gallery]"""
    q, e, dtype, alpha = ROUTES[route]
    n_img, n_txt = (N_GAL, N_QRY) if kind == "image" else (N_QRY, N_GAL)
    img_f, txt_f = R.features(n_img, e, 1), R.features(n_txt, e, 2)
    img_t, txt_t = R.image_tokens(n_img, q, e, 3, dtype), R.text_tokens(n_txt, 20, e, 4, dtype)
    tok = R.einsum_ref(img_t.double(), txt_t.double())                               # [n_txt, n_img]
    dense = SCALE * (alpha * (txt_f.double() @ img_f.double().t()) + (1 - alpha) * tok)
    dense = dense if kind == "image" else dense.t()
    gal, qry = ((img_f, img_t), (txt_f, txt_t)) if kind == "image" else ((txt_f, txt_t), (img_f, img_t))
    return gal, qry, dense, alpha


def _index(kind, route, monkeypatch):
    monkeypatch.setattr(LateInteractionIndex, "CHUNK_ITEMS", 16)
    monkeypatch.setattr(LateInteractionIndex, "QUERY_CHUNK", 8)
    (gal_f, gal_t), (qry_f, qry_t), dense, alpha = _case(kind, route)
    ids = 1000 + 3 * torch.arange(N_GAL)
    index = LateInteractionIndex(kind, alpha=alpha, scale=SCALE, device=DEV)
    index.add(gal_f[:20].to(DEV), gal_t[:20].to(DEV), ids=ids[:20])
    index.add(gal_f[20:].to(DEV), gal_t[20:].to(DEV), ids=ids[20:])
    assert [c[1].shape[0] for c in index.chunks()] == [16, 16, 3]
    return index, qry_f.to(DEV), qry_t.to(DEV), dense, ids


def _ids_of(pos, ids):
    return torch.where(pos >= 0, ids[pos.clamp(min=0).long()], torch.full_like(pos, -1).long())


@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("kind", ["image", "text"])
def test_rerank(kind, route, monkeypatch):
    index, qf, qt, dense, ids = _index(kind, route, monkeypatch)
    calls = _spy(monkeypatch)
    C = 12
    pos = _candidates(N_QRY, C, seed=23)
    pos[5, :3] = torch.tensor([4, 4, 30])
    pos[5, 3:] = -1                                                                  # a query with three candidates, one twice
    scores = index.rerank(qf, qt, pos.to(DEV))
    assert scores.shape == (N_QRY, C) and scores.dtype == torch.float32 and scores.is_cuda
    assert calls == ([(8, C), (8, C), (3, C)] if route == "fused_bf16" else [])      # per query chunk
    ref = dense.gather(1, pos.clamp(min=0))
    ref[pos < 0] = -INF
    err = _check(scores, ref, pos, SCALE * BOUND, (kind, route))
    print(f"rerank {kind} gallery, {route}: max |score - fp64| = {err:.3e} at scale {SCALE}")
    assert err <= SCALE * BOUND, err
    for k in (5, 14):
        val, got_ids = index.rerank(qf, qt, pos.to(DEV), k)
        want_v, want_p = topk_reference(torch.empty(N_QRY, 0), k, 0, best=(scores, pos))
        assert got_ids.dtype == torch.int64 and torch.equal(got_ids.cpu(), _ids_of(want_p, ids)), (kind, route, k)
        assert torch.equal(_bits(val.cpu()), _bits(want_v)), (kind, route, k)
    live = int((pos[5] >= 0).sum())
    assert live == 3 and bool((got_ids[5, live:] == -1).all()) and bool((val[5, live:] == -INF).all())
    if kind == "text" and route == "fused_bf16":     # the packed-row counts stay beside the chunks until add touches one
        assert sorted(index._pair_cnt) == [0, 1, 2]
        (gal_f, gal_t), _, _, _ = _case(kind, route)
        index.add(gal_f[:1].to(DEV), gal_t[:1].to(DEV), ids=torch.tensor([7]))
        assert sorted(index._pair_cnt) == [0, 1]
        again = index.rerank(qf, qt, pos.to(DEV))
        assert torch.equal(_bits(again), _bits(scores)) and index._pair_cnt[2].shape[0] == 4


# ------------------------------------------------------------------------------------------------ 5. search(candidates=C)
def _returned_is_top(val, got_ids, ref, ids, k, bound, what):
    """`ref` [nq, gallery] fp64 with -inf outside the candidate set: each returned score lies within `bound` of the reference of
    its id, the list is non-increasing, and every item whose reference beats the k-th returned score by more than 2 * bound is
    in it"""
    val, got_ids = val.cpu().double(), got_ids.cpu()
    pos_of = {int(i): p for p, i in enumerate(ids.tolist())}
    assert set(got_ids.flatten().tolist()) <= set(ids.tolist()) | {-1}, what
    worst = 0.0
    for j in range(val.shape[0]):
        row = [(float(v), int(i)) for v, i in zip(val[j], got_ids[j]) if int(i) != -1]
        assert len(row) == min(k, int((ref[j] > -INF).sum())), what
        assert all(a[0] >= b[0] for a, b in zip(row, row[1:])), what
        for v, i in row:
            worst = max(worst, abs(v - float(ref[j, pos_of[i]])))
        if len(row) == k:
            must = (ref[j] > row[-1][0] + 2 * bound).nonzero().flatten().tolist()
            assert {int(ids[p]) for p in must} <= {i for _, i in row}, (what, j)
    assert worst <= bound, (what, worst)
    return worst


@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("kind", ["image", "text"])
def test_search_with_candidates(kind, route, monkeypatch):
    index, qf, qt, dense, ids = _index(kind, route, monkeypatch)
    (gal_f, _), _, _, _ = _case(kind, route)
    gal_f = gal_f.to(DEV)
    # the global similarities over the same chunk boundaries (8 queries x 16 items), queries x gallery
    G = torch.empty(N_QRY, N_GAL, device=DEV)
    for q0 in range(0, N_QRY, 8):
        for g0 in range(0, N_GAL, 16):
            a, b = qf[q0:q0 + 8], gal_f[g0:g0 + 16]
            G[q0:q0 + 8, g0:g0 + 16] = TR.similarity_matrix(b, a).t() if kind == "image" else TR.similarity_matrix(a, b)
    seen = []
    real = LateInteractionIndex.rerank
    monkeypatch.setattr(LateInteractionIndex, "rerank", lambda self, f, t, p, k=None, global_scores=None:
                        (seen.append((p.clone(), global_scores.clone())), real(self, f, t, p, k, global_scores=global_scores))[1])
    merges = []
    merge = ops.topk_merge
    monkeypatch.setattr(ops, "topk_merge", lambda s, qd, base, bv, bi: (merges.append((tuple(s.shape), qd, base)), merge(s, qd, base, bv, bi))[1])
    scored = []
    for name in ("maxsim_scores", "maxsim_scores_fp8"):
        monkeypatch.setattr(ops, name, lambda *a, **kw: scored.append(1))
    for C, k in ((40, 5), (40, 40), (8, 5), (8, 8)):
        seen.clear(), merges.clear()
        val, got_ids = index.search(qf, qt, k, candidates=C)
        assert val.shape == (N_QRY, k) and got_ids.dtype == torch.int64 and not scored           # no dense token scoring
        want_v, want_p = topk_reference(G.cpu(), C, 0)
        (p, g), = seen
        assert torch.equal(p.cpu(), want_p) and torch.equal(_bits(g.cpu()), _bits(want_v))       # the candidate sets, exactly
        stage1 = [(m[0][0] if kind == "image" else m[0][1], m[2]) for m in merges[:-1]]
        assert stage1 == [(16, 0), (16, 16), (3, 32)] * 3 and merges[-1][0] == (N_QRY, C)
        again = real(index, qf, qt, want_p.to(DEV), k, global_scores=want_v.to(DEV))             # rerank on those positions
        assert torch.equal(got_ids, again[1]) and torch.equal(_bits(val), _bits(again[0]))
        own = real(index, qf, qt, want_p.to(DEV))                                                # ... with rerank's own global term
        given = real(index, qf, qt, want_p.to(DEV), global_scores=want_v.to(DEV))
        live = want_p >= 0
        assert float((own.cpu() - given.cpu())[live].abs().max()) <= SCALE * BOUND
        ref = torch.full_like(dense, -INF)
        ref.scatter_(1, want_p.clamp(min=0).long(), dense.gather(1, want_p.clamp(min=0).long()))
        if C >= N_GAL:
            assert bool((ref == dense).all())                                                    # every item is a candidate
        worst = _returned_is_top(val, got_ids, ref, ids, k, SCALE * BOUND, (kind, route, C, k))
        print(f"search(candidates={C}) {kind} gallery, {route}, k={k}: max |score - fp64| = {worst:.3e} at scale {SCALE}")
    assert bool((val[:, 0] > -INF).all())


# ------------------------------------------------------------------------------------------------ 6. through a model and the CLI
NAME = R.Q49_MODEL


def test_candidates_through_a_model_and_the_cli(tmp_path):
    """ViT-q49-test-colxlip in bf16 on a synthetic retrieval split of 16 images x 5 captions: `search_texts(candidates=8)` over an
    index filled batch by batch as the command line fills it, and `python -m colxlip_amd.search --candidates 8`: the same ids."""
    model = R.build_model(NAME, R.model_state(Q49), "bf16").eval()
    ckpt = str(tmp_path / "model.pt")
    torch.save({"state_dict": {k: v.detach().cpu() for k, v in model.state_dict().items()}}, ckpt)
    argv = ["--model", NAME, "--dataset-type", "synthetic", "--precision", "bf16", "--batch-size", "16", "--retrieval-coco",
            "--val-num-samples", "16", "--alpha", "0.5", "--k", "5", "--candidates", "8"]
    args = S.parse_args(argv)
    args.rank, args.local_rank, args.world_size, args.distributed, args.device = 0, 0, 1, False, "cuda"
    args.save_logs, args.wandb = False, False
    data = get_data(args, model=model)
    txt, img, _, _ = data["retrieval_coco"]
    index = LateInteractionIndex.from_model(model, "image", alpha=0.5)
    for batch, ids in img.dataloader:
        index.add_images(model, batch.to(device=DEV, dtype=torch.bfloat16), ids=torch.as_tensor(ids).reshape(-1))
    found = []
    for batch, _ in txt.dataloader:
        batch = batch.to(DEV)
        batch = (batch[:, 0] if batch.ndim == 3 else batch).contiguous()
        found.append(index.search_texts(model, batch, 5, candidates=8)[1])
    found = torch.cat(found).cpu().numpy()
    assert found.shape == (80, 5) and set(found.flatten().tolist()) <= set(index.ids.tolist())
    del model
    out = str(tmp_path / "results.npz")
    cmd = [sys.executable, *(["-s"] if sys.flags.no_user_site else []), "-c", R.LAUNCHER, ROOT, *argv, "--pretrained", ckpt,
           "--direction", "t2i", "--out", out]
    done = subprocess.run(cmd, cwd=str(tmp_path), capture_output=True, text=True, timeout=300)
    assert done.returncode == 0, done.stderr[-2000:]
    z = np.load(out, allow_pickle=False)
    assert z["ids"].shape == (80, 5) and np.array_equal(z["ids"], found)
    assert bool((z["scores"][:, :-1] >= z["scores"][:, 1:]).all())


# ------------------------------------------------------------------------------------------------ 7. memory
def test_peak_memory_with_candidates_does_not_grow_with_the_gallery(monkeypatch):
    """The method of test_search_gpu.py: 64 queries, k = 10, C = 16, gallery chunks of 256 items; what `search(candidates=16)`
    allocates above what is live before it is the same, within 64 KiB, for 2 048 and 4 096 gallery items."""
    monkeypatch.setattr(LateInteractionIndex, "CHUNK_ITEMS", 256)
    e = 128
    qf, qt = R.features(64, e, 2).to(DEV), R.text_tokens(64, 20, e, 4, torch.bfloat16).to(DEV)
    peaks = []
    for n in (2048, 4096):
        index = LateInteractionIndex("image", alpha=0.5, scale=10.0, device=DEV)
        index.add(R.features(n, e, 1).to(DEV), R.image_tokens(n, 16, e, 3, torch.bfloat16).to(DEV))
        index.search(qf, qt, 10, candidates=16)                    # warm: library handles, kernel attributes
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        live = torch.cuda.memory_allocated()
        val, ids = index.search(qf, qt, 10, candidates=16)
        torch.cuda.synchronize()
        peaks.append(torch.cuda.max_memory_allocated() - live)
        assert int(ids.max()) < n and int(ids.min()) >= 0
        del index, val, ids
    print(f"search(candidates=16) peak above live memory: {peaks[0]} B at 2048 items, {peaks[1]} B at 4096 items")
    assert abs(peaks[1] - peaks[0]) <= 64 * 1024, peaks


# ------------------------------------------------------------------------------------------------ 8. refusals
def test_refusals_launch_nothing_and_change_no_state(monkeypatch):
    index, qf, qt, _, _ = _index("text", "fused_bf16", monkeypatch)
    calls = _spy(monkeypatch)
    launched = []
    for name in ("topk_merge", "maxsim_text_counts", "maxsim_scores", "gemm_f32"):
        monkeypatch.setattr(ops, name, lambda *a, _n=name, **kw: launched.append(_n))
    pos = _candidates(N_QRY, 6, seed=2).to(DEV)
    far = pos.clone()
    far[3, 4] = N_GAL                                                                # == len(index)
    wide = torch.zeros(N_QRY, 12, dtype=torch.int64, device=DEV)
    one = LateInteractionIndex("text", alpha=1.0, scale=2.0, device=DEV).add(R.features(5, 128, 1).to(DEV))
    pre = LateInteractionIndex("text", alpha=1.0, scale=2.0, device=DEV, prescale=True).add(R.features(5, 128, 1).to(DEV))
    for case, match in ((lambda: index.search(qf, qt, 5, candidates=4), "candidates"),
                        (lambda: index.search(qf, qt, 5, candidates=257), "candidates"),
                        (lambda: one.search(qf, None, 2, candidates=4), "alpha = 1"),
                        (lambda: pre.search(qf, None, 2, candidates=4), "alpha = 1"),
                        (lambda: one.rerank(qf, qt, pos), "alpha = 1"),
                        (lambda: index.rerank(qf, qt, far), "outside"),
                        (lambda: index.rerank(qf, qt, wide[:, ::2]), "contiguous")):
        with pytest.raises(ValueError, match=match):
            case()
    assert calls == [] and launched == [] and len(index) == N_GAL and index._pair_cnt == {}
    monkeypatch.undo()
    # an fp8 index (filled on the device): refused before anything is quantised or scored
    fp8 = LateInteractionIndex("image", alpha=0.4, scale=2.0, device=DEV, token_dtype="fp8")
    fp8.add(R.features(5, 256, 1).to(DEV), R.image_tokens(5, 16, 256, 3).to(DEV))
    calls = _spy(monkeypatch)
    monkeypatch.setattr(ops, "quant_tokens_e4m3", lambda *a: pytest.fail("the queries were quantised"))
    monkeypatch.setattr(ops, "dequant_tokens_e4m3", lambda *a, **kw: pytest.fail("the gallery was dequantised"))
    for case in (lambda: fp8.search(R.features(3, 256, 2).to(DEV), R.text_tokens(3, 20, 256, 4).to(DEV), 2, candidates=4),
                 lambda: fp8.rerank(R.features(3, 256, 2).to(DEV), R.text_tokens(3, 20, 256, 4).to(DEV), torch.zeros(3, 2, dtype=torch.int64))):
        with pytest.raises(ValueError, match="fp8"):
            case()
    assert calls == []


def test_entry_refuses_bad_counts_and_positions():
    """What only the device knows -- a cnt outside 1 .. n, a position outside the gallery -- is found by the entry's read-only
    pass: the call fails and `out` keeps what it held."""
    q, n, e = 49, 20, 128
    ti, tt, _ = _sides(q, n, e, 33, N_GAL)
    gal, qry = tt.to(DEV), ti[:4].to(DEV)
    cand = _candidates(4, 6, seed=8).to(DEV)
    cand[1, 3] = 20
    good = [ops.maxsim_text_counts(c) for c in _chunks(gal)]
    out = torch.full((4, 6), 7.0, device=DEV)
    for bad_value in (0, n + 1, -3):
        cnts = [c.clone() for c in good]
        cnts[1][4] = bad_value                                                       # position 20 = chunk 1, item 4
        with pytest.raises(RuntimeError, match="cnt lies outside"):
            ops.maxsim_pair_scores(qry, list(zip(_chunks(gal), cnts)), CHUNK, cand, None, 0.0, 1.0, False, out=out)
        assert bool((out == 7.0).all())
    cnts = [c.clone() for c in good]
    cnts[1][5] = 0                                                                   # a bad cnt no candidate names is not looked at
    cand[cand == 21] = 22
    ops.maxsim_pair_scores(qry, list(zip(_chunks(gal), cnts)), CHUNK, cand, None, 0.0, 1.0, False, out=out)
    assert bool((out != 7.0).all())
    out.fill_(7.0)
    for bad_value in (N_GAL, -2, 2 ** 31 - 1):
        far = cand.clone()
        far[2, 0] = bad_value
        with pytest.raises(RuntimeError, match="position lies outside"):
            ops.maxsim_pair_scores(qry, list(zip(_chunks(gal), good)), CHUNK, far, None, 0.0, 1.0, False, out=out)
        assert bool((out == 7.0).all())
