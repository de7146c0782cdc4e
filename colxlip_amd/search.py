"""Late-interaction search: the k best gallery items per query, without the dense score matrix.

`LateInteractionIndex` owns the features of one side (the gallery) on the device.  `search` walks (query chunk x gallery chunk):
the global similarities of the pair are one fp32 GEMM (`train.similarity_matrix`), `ops.maxsim_scores` writes the pair's score
tile into a buffer that is allocated once per search, and `ops.topk_merge` (`clipx_topk_merge`, csrc/topk.hip) folds the tile into
the running k best of every query.  The scores are those of `ColXLIP.get_logits` / `train.evaluate` (the reference's
arithmetic); the selection replaces the reference's per-row CPU argsort (train.py:457-508), which needs every score in memory.

    python -m colxlip_amd.search --model NAME [--pretrained CKPT] [--precision bf16] --dataset-type synthetic|packed
        [--val-data DIR] --retrieval-coco --direction t2i|i2t --k 10 --out results.npz [--save-index DIR | --load-index DIR]
        [--index-dtype model|fp8] [--candidates C]

`token_dtype="fp8"` keeps the gallery's token features as e4m3 bytes with one power-of-two exponent per token
(`ops.quant_tokens_e4m3`): half the bytes of bf16 plus 4 per token, scored by `ops.maxsim_scores_fp8` on the fp8 MFMA.
"""
import json
import logging
import math
import os

import numpy as np
import torch

from . import ops

_FILES = ("meta.json", "features.npy", "tokens.npy", "ids.npy")
_FP8_FILES = ("token_exp.npy", "token_cnt.npy")     # beside tokens.npy (uint8) of an fp8 index; token_cnt.npy: text galleries only


def topk_reference(scores, k, query_dim, c_base=0, best=None):
    """The selection of `ops.topk_merge` in plain torch, on the CPU: (values [nq, k] fp32, positions [nq, k] int32) of the k best
    candidates per query under (larger value first, then smaller gallery position), by stable sorts.  `scores` is 2-D, dimension
    `query_dim` indexes the queries and the other one gallery positions c_base, c_base + 1, ...; -inf and NaN candidates are
    skipped, missing entries are (-inf, -1).  `best` = (values, positions) of an earlier call joins the candidates."""
    s = scores.detach().cpu().float()
    s = s if query_dim == 0 else s.t()
    nq, nc = s.shape
    val = s.clone()
    pos = (torch.arange(nc, dtype=torch.int64) + int(c_base)).expand(nq, nc).clone()
    if best is not None:
        val = torch.cat([best[0].detach().cpu().float(), val], dim=1)
        pos = torch.cat([best[1].detach().cpu().to(torch.int64), pos], dim=1)
    dead = torch.isnan(val) | (val == float("-inf"))
    val[dead] = float("-inf")
    pos[dead] = -1
    order = torch.sort(pos, dim=1, stable=True)[1]                       # smaller position first ...
    val, pos = val.gather(1, order), pos.gather(1, order)
    order = torch.sort(val, dim=1, descending=True, stable=True)[1]      # ... among equal values
    val, pos = val.gather(1, order), pos.gather(1, order)
    out_v = torch.full((nq, k), float("-inf"), dtype=torch.float32)
    out_i = torch.full((nq, k), -1, dtype=torch.int32)
    m = min(k, val.shape[1])
    out_v[:, :m] = val[:, :m]
    out_i[:, :m] = pos[:, :m].to(torch.int32)
    return out_v, out_i


def image_chunk_items(limit, q):
    """Images per chunk of the scorer's image operand: at most `limit` and `ops.MAXSIM_MAX_IMAGES`, a multiple of the unit that
    makes (ci * q) % 8 == 0 (the MaxSim GEMM's alignment), so that only a last, partial chunk is ever padded."""
    unit = 8 // math.gcd(int(q), 8)
    return max(unit, min(int(limit), ops.MAXSIM_MAX_IMAGES) // unit * unit)


def _to_numpy(t):
    """(array, dtype name): bf16 travels as its uint16 bit patterns"""
    t = t.detach().cpu().contiguous()
    if t.dtype == torch.bfloat16:
        return t.view(torch.int16).numpy().view(np.uint16), "bfloat16"
    return t.numpy(), str(t.dtype).replace("torch.", "")


def _from_numpy(a, dtype_name):
    a = np.array(a)                                  # a writable copy (the source may be a read-only memory map)
    if dtype_name == "bfloat16":
        return torch.from_numpy(a.view(np.int16)).view(torch.bfloat16)
    return torch.from_numpy(a)


class LateInteractionIndex:
    """A gallery of images (`kind="image"`, queried with texts) or of texts (`kind="text"`, queried with images), scored by
        scale * (alpha * global + (1 - alpha) * MaxSim(tokens))
    as `ops.maxsim_scores` computes it.  `prescale` moves the scale onto the image features BEFORE the similarity GEMM,
    (scale * I) T^T, which is how a plain CLIP model forms its logits (reference train.py:608); it needs alpha = 1.
    A model's logit_bias is not part of the scores: a constant does not change a ranking.

    `token_dtype=None` stores the tokens as they come; `token_dtype="fp8"` stores e4m3 bytes [chunk, q, E] uint8 with exponents
    [chunk, q] int32 (`ops.quant_tokens_e4m3`), for a text gallery also cnt [chunk] int32 (`ops.maxsim_text_counts` of the bf16
    rows), and scores both directions with `ops.maxsim_scores_fp8`: MaxSim of the dequantised tokens."""

    CHUNK_ITEMS = 16384          # gallery items per chunk (storage and scoring)
    QUERY_CHUNK = 8192           # queries per chunk: the score tile is at most CHUNK_ITEMS x QUERY_CHUNK x 4 bytes
    IO_ITEMS = 65536             # items per copy of save / load

    def __init__(self, kind="image", alpha=0.5, scale=1.0, device="cuda", prescale=False, token_dtype=None):
        if kind not in ("image", "text"):
            raise ValueError(f"LateInteractionIndex: kind must be 'image' or 'text' (got {kind!r})")
        if token_dtype not in (None, "fp8"):
            raise ValueError(f"LateInteractionIndex: token_dtype must be None (the model's dtype) or 'fp8' (got {token_dtype!r})")
        self.token_dtype = token_dtype
        if prescale and float(alpha) != 1.0:
            raise ValueError("LateInteractionIndex: prescale is the plain CLIP form of the logits and needs alpha = 1")
        self.kind, self.alpha, self.scale, self.prescale = kind, float(alpha), float(scale), bool(prescale)
        self.device = torch.device(device)
        self._feat, self._tok = [], []           # chunks [chunk, E] fp32 / [chunk, q, E]; the last one may be partly filled
        self._tok_exp, self._tok_cnt = [], []    # fp8: chunks [chunk, q] int32 / (text gallery) [chunk] int32 beside the bytes in _tok
        self._pair_cnt = {}                      # bf16 text gallery, rerank: chunk number -> cnt [items] int32 (ops.maxsim_text_counts)
        self._ids = torch.empty((0,), dtype=torch.int64, device=self.device)      # capacity doubles
        self._n = 0
        self._chunk = None                       # items per chunk, fixed by the first add
        self._running_ids = True                 # ids are the positions: search skips the gather

    def __len__(self):
        return self._n

    @property
    def has_tokens(self):
        return bool(self._tok)

    @property
    def ids(self):
        return self._ids[:self._n]

    # ------------------------------------------------------------------ storage
    def _plan_chunk(self, tokens):
        if self.kind == "image" and tokens is not None:
            return image_chunk_items(self.CHUNK_ITEMS, tokens.shape[1])
        return max(1, int(self.CHUNK_ITEMS))

    def add(self, features, tokens=None, ids=None):
        """features [n, E] fp32, normalised; tokens [n, q, E] in the model's compute dtype (None: a model without token features,
        alpha must be 1); ids int64 [n] (default: the running position).  Storage grows by chunks of `CHUNK_ITEMS` items; only the
        last, partly filled chunk is ever copied (it doubles up to a full chunk).
        An fp8 index takes the same bf16 tokens and quantises them as they arrive; fp32 tokens are cast to bf16 first, which
        ROUNDS them (8 significant bits) before the e4m3 step.  It also takes the stored form itself, (bytes, exp) or for a text
        gallery (bytes, exp, cnt), as `chunks` yields it: that is kept byte for byte (`load` uses it)."""
        n = features.shape[0]
        if features.dim() != 2 or features.dtype != torch.float32:
            raise ValueError("LateInteractionIndex.add: features must be [n, E] fp32")
        if self.alpha == 1.0:
            tokens = None                        # never read
        elif tokens is None:
            raise ValueError("LateInteractionIndex.add: alpha != 1 scores with token features; pass tokens or use alpha = 1")
        extra = ()                               # fp8: (exp [n, q],) or (exp, cnt [n]) beside the bytes
        if tokens is not None and self.token_dtype == "fp8":
            tokens, *extra = self._quantise(tokens, n)
        if tokens is not None and (tokens.dim() != 3 or tokens.shape[0] != n or tokens.shape[2] != features.shape[1]):
            raise ValueError("LateInteractionIndex.add: tokens must be [n, q, E] with the features' n and E")
        if self._n and tokens is not None and (tokens.shape[1:] != self._tok[0].shape[1:] or tokens.dtype != self._tok[0].dtype):
            raise ValueError("LateInteractionIndex.add: token shape or dtype differs from the stored ones")
        if self._n and features.shape[1] != self._feat[0].shape[1]:
            raise ValueError("LateInteractionIndex.add: embed dim differs from the stored one")
        if ids is None:
            ids = torch.arange(self._n, self._n + n, dtype=torch.int64)
        else:
            ids = torch.as_tensor(ids, dtype=torch.int64).reshape(-1)
            if ids.numel() != n:
                raise ValueError("LateInteractionIndex.add: one id per item")
            self._running_ids = False
        if self._chunk is None:
            self._chunk = self._plan_chunk(tokens)
        if self._n + n > self._ids.numel():
            grown = torch.empty((max(2 * self._ids.numel(), self._n + n, 1024),), dtype=torch.int64, device=self.device)
            grown[:self._n] = self._ids[:self._n]
            self._ids = grown
        self._ids[self._n:self._n + n] = ids.to(self.device)
        done = 0
        while done < n:
            fill = self._n % self._chunk
            want = min(self._chunk, fill + n - done)             # items of the last chunk after this round
            have = self._feat[-1].shape[0] if fill else 0
            if have < want:                                      # a new chunk, or the last one grows (doubling, up to a full chunk)
                cap = min(self._chunk, max(want, 2 * have))
                feat = torch.empty((cap, features.shape[1]), dtype=torch.float32, device=self.device)
                tok = None if tokens is None else torch.empty((cap,) + tuple(tokens.shape[1:]), dtype=tokens.dtype, device=self.device)
                side = [torch.empty((cap,) + tuple(x.shape[1:]), dtype=torch.int32, device=self.device) for x in extra]
                if fill:
                    feat[:fill] = self._feat.pop()[:fill]
                    if tok is not None:
                        tok[:fill] = self._tok.pop()[:fill]
                    for new, store in zip(side, (self._tok_exp, self._tok_cnt)):
                        new[:fill] = store.pop()[:fill]
                self._feat.append(feat)
                if tok is not None:
                    self._tok.append(tok)
                for new, store in zip(side, (self._tok_exp, self._tok_cnt)):
                    store.append(new)
            take = want - fill
            self._feat[-1][fill:want] = features[done:done + take].detach().to(self.device)
            if tokens is not None:
                self._tok[-1][fill:want] = tokens[done:done + take].detach().to(self.device)
            for x, store in zip(extra, (self._tok_exp, self._tok_cnt)):
                store[-1][fill:want] = x[done:done + take].to(self.device)
            self._pair_cnt.pop(len(self._feat) - 1, None)        # the chunk changed: its counts are recomputed when next needed
            done += take
            self._n += take
        return self

    def _quantise(self, tokens, n):
        """tokens of an fp8 index -> (bytes [n, q, E] uint8, exp [n, q] int32[, cnt [n] int32 for a text gallery]) on the device"""
        want = 3 if self.kind == "text" else 2
        if isinstance(tokens, (tuple, list)):                    # the stored form, kept as it is
            if len(tokens) != want or tokens[0].dtype != torch.uint8 or any(x.dtype != torch.int32 for x in tokens[1:]):
                raise ValueError(f"LateInteractionIndex.add: the stored form of {self.kind} tokens is "
                                 f"(bytes uint8, exp int32{', cnt int32' if want == 3 else ''})")
            if tokens[0].dim() != 3 or tokens[1].shape != tokens[0].shape[:2] or (want == 3 and tokens[2].shape != tokens[0].shape[:1]):
                raise ValueError("LateInteractionIndex.add: bytes [n, q, E], exp [n, q] and cnt [n] must agree")
            return tuple(x.detach().to(self.device) for x in tokens)
        if tokens.dtype not in (torch.bfloat16, torch.float32):
            raise ValueError("LateInteractionIndex.add: token dtype differs from the stored ones: an fp8 index takes bf16 tokens "
                             "(or fp32, rounded to bf16)")
        if tokens.dim() != 3 or tokens.shape[0] != n:
            raise ValueError("LateInteractionIndex.add: tokens must be [n, q, E] with the features' n and E")
        return self._scorer_form(tokens, self.kind)

    def _scorer_form(self, tokens, side):
        """tokens [n, q, E] of `side` ("image" or "text") -> on the device, in the form the scorer takes: as they are, or for an fp8
        index (bytes, exp) of their bf16 cast, for a text side (bytes, exp, cnt)"""
        tokens = tokens.detach().to(self.device)
        if self.token_dtype != "fp8":
            return tokens
        tokens = tokens.to(torch.bfloat16).contiguous()
        out = ops.quant_tokens_e4m3(tokens)
        return out + (ops.maxsim_text_counts(tokens),) if side == "text" else out

    def chunks(self):
        """[(position of the first item, features [n, E], tokens [n, q, E] or None)] over the stored items; an fp8 index yields
        its stored form in the place of the tokens: (bytes [n, q, E], exp [n, q]), for a text gallery (bytes, exp, cnt [n])"""
        out = []
        for c, feat in enumerate(self._feat):
            base = c * self._chunk
            n = min(self._chunk, self._n - base)
            tok = self._tok[c][:n] if self._tok else None
            if tok is not None and self.token_dtype == "fp8":
                tok = (tok, self._tok_exp[c][:n]) + ((self._tok_cnt[c][:n],) if self.kind == "text" else ())
            out.append((base, feat[:n], tok))
        return out

    def token_bytes(self):
        """bytes of the stored token tensors (an fp8 index: bytes, exponents and counts), whole chunks as allocated"""
        return sum(t.numel() * t.element_size() for store in (self._tok, self._tok_exp, self._tok_cnt) for t in store)

    # ------------------------------------------------------------------ search
    def search(self, features, tokens, k, candidates=None):
        """features [nq, E] fp32 (normalised), tokens [nq, n, E] or None (alpha = 1) of the OTHER side -> (scores [nq, k] fp32,
        ids [nq, k] int64) on the device, best first (larger score, then earlier gallery position); slots beyond the gallery
        size hold (-inf, -1).  Nothing of size gallery x queries is allocated.  An fp8 index quantises the query tokens once per
        query chunk (fp32 ones are cast to bf16 first) and scores with `ops.maxsim_scores_fp8`; no bf16 copy of a gallery chunk
        is made.
        `candidates=C` (k <= C <= ops.TOPK_MAX_K) searches in two stages: the C best gallery items per query by the GLOBAL
        similarity alone (the same loop with `similarity_matrix` merged directly, no token kernel), then `rerank` of those
        positions with the full score, reusing the first stage's global similarities.  The result is the exact top k of the
        candidates, not of the gallery; with C >= len(self) it is the exhaustive result up to summation order."""
        if candidates is not None and candidates != 0:
            return self._search_two_stage(features, tokens, k, int(candidates))
        nq = features.shape[0]
        dev = self.device
        if self.alpha == 1.0:
            tokens = None
        elif tokens is None or not self._tok and self._n:
            raise ValueError("LateInteractionIndex.search: alpha != 1 needs token features on both sides")
        features = features.detach().to(dev).float().contiguous()
        best_val, best_idx = ops.topk_init(nq, k, dev)
        if nq == 0 or self._n == 0:
            return best_val, best_idx.to(torch.int64)
        gallery_is_image = self.kind == "image"
        qchunk = max(1, int(self.QUERY_CHUNK))
        if not gallery_is_image and tokens is not None:
            qchunk = image_chunk_items(qchunk, tokens.shape[1])
        qchunk = min(qchunk, nq)
        gchunk = min(self._chunk, self._n)
        tile = torch.empty((gchunk, qchunk) if gallery_is_image else (qchunk, gchunk), dtype=torch.float32, device=dev)
        s_dev = torch.tensor([self.scale], dtype=torch.float32, device=dev) if self.prescale else None
        scale = 1.0 if self.prescale else self.scale
        from .train import similarity_matrix
        score = ops.maxsim_scores_fp8 if self.token_dtype == "fp8" else ops.maxsim_scores      # looked up per search
        with torch.no_grad():
            for q0 in range(0, nq, qchunk):
                q1 = min(nq, q0 + qchunk)
                qf = features[q0:q1]
                qt = None if tokens is None else self._scorer_form(tokens[q0:q1], "text" if gallery_is_image else "image")
                for base, gf, gt in self.chunks():
                    n = gf.shape[0]
                    img_f, img_t, txt_f, txt_t = (gf, gt, qf, qt) if gallery_is_image else (qf, qt, gf, gt)
                    view = tile[:n, :q1 - q0] if gallery_is_image else tile[:q1 - q0, :n]
                    if s_dev is not None:
                        img_f = ops.scale_by_dev(img_f.contiguous(), s_dev)
                    G = similarity_matrix(img_f, txt_f)
                    score(img_t, txt_t, G, self.alpha, scale, out=view)
                    ops.topk_merge(view, 1 if gallery_is_image else 0, base, best_val[q0:q1], best_idx[q0:q1])
        pos = best_idx.to(torch.int64)
        if self._running_ids:
            return best_val, pos
        found = self._ids[:self._n][pos.clamp_(min=0)]
        return best_val, torch.where(best_idx >= 0, found, torch.full_like(found, -1))

    # ------------------------------------------------------------------ two-stage search and reranking
    def _refuse_rerank(self, what):
        if self.alpha == 1.0 or self.prescale:
            raise ValueError(f"LateInteractionIndex.{what}: alpha = 1 (or prescale) scores with the global features alone; the exact "
                             "search is already the global one, there is nothing to rerank")
        if self.token_dtype == "fp8":
            raise ValueError(f"LateInteractionIndex.{what}: an fp8 token index is not reranked (the gathered MaxSim kernel reads bf16 "
                             "tokens; dequantising the gallery is not done silently)")

    def _pair_chunks(self):
        """the token storage as `ops.maxsim_pair_scores` takes it: the chunks' filled parts, a bf16 text gallery's with their cnt"""
        out = []
        for c, (base, _, tok) in enumerate(self.chunks()):
            if self.kind == "text" and tok.dtype == torch.bfloat16:
                cnt = self._pair_cnt.get(c)
                if cnt is None or cnt.shape[0] != tok.shape[0]:
                    cnt = self._pair_cnt[c] = ops.maxsim_text_counts(tok)
                out.append((tok, cnt))
            else:
                out.append(tok)
        return out

    def _pair_globals(self, qf, pos):
        """fp32 global similarities of the pairs (qf [m, E], pos [m, C] int64, -1 = empty): [m, C], 0 at empty slots; the gallery
        features are gathered chunk by chunk, 64 MiB of them at a time"""
        m, C = pos.shape
        e = qf.shape[1]
        out = torch.zeros((m, C), dtype=torch.float32, device=self.device)
        step = max(1, (64 << 20) // max(1, 4 * C * e))
        for a in range(0, m, step):
            p = pos[a:a + step]
            rows = torch.arange(a, a + p.shape[0], device=self.device).unsqueeze(1).expand_as(p)
            for base, gf, _ in self.chunks():
                hit = (p >= base) & (p < base + gf.shape[0])
                out[a:a + step][hit] = (gf[p[hit] - base] * qf[rows[hit]]).sum(-1)
        return out

    def rerank(self, features, tokens, positions, k=None, global_scores=None):
        """The full scores of chosen candidates: features [nq, E] fp32 and tokens [nq, n, E] of the queries, positions [nq, C] int
        (gallery POSITIONS, -1 = an empty slot; duplicates are scored as given).  k None -> scores [nq, C] fp32 in the given slot
        order, -inf at empty slots.  With k -> (scores [nq, k], ids [nq, k] int64) best first under the index's order (larger
        score, then smaller gallery position), positions mapped through `ids` as `search` does, (-inf, -1) behind the last
        candidate.  The global term comes from the fp32 features of the pairs, or from `global_scores` [nq, C] fp32 when the
        caller has them (`search(candidates=C)` passes its first stage's).  Scoring is `ops.maxsim_pair_scores` per query chunk."""
        self._refuse_rerank("rerank")
        if tokens is None or not self._tok and self._n:
            raise ValueError("LateInteractionIndex.rerank: needs token features on both sides")
        positions = torch.as_tensor(positions)
        if positions.dim() != 2 or positions.shape[0] != features.shape[0] or positions.dtype not in (torch.int32, torch.int64):
            raise ValueError("LateInteractionIndex.rerank: positions must be [nq, C] int32 or int64")
        nq, C = positions.shape
        if (C > 1 and positions.stride(1) != 1) or (nq > 1 and positions.stride(0) != C):
            raise ValueError("LateInteractionIndex.rerank: positions must be contiguous")
        if k is not None and not 1 <= k <= ops.TOPK_MAX_K:
            raise ValueError(f"LateInteractionIndex.rerank: k must be in 1 .. {ops.TOPK_MAX_K} (got {k})")
        dev = self.device
        positions = positions.to(dev)
        if positions.numel() and (int(positions.max()) >= self._n or int(positions.min()) < -1):
            raise ValueError(f"LateInteractionIndex.rerank: a position lies outside [0, {self._n}) and is not -1")
        if global_scores is not None and (global_scores.shape != positions.shape or global_scores.dtype != torch.float32):
            raise ValueError("LateInteractionIndex.rerank: global_scores must be [nq, C] fp32")
        features = features.detach().to(dev).float().contiguous()
        tokens = tokens.detach().to(dev)
        scores = torch.empty((nq, C), dtype=torch.float32, device=dev)
        gallery_is_image = self.kind == "image"
        qchunk = max(1, int(self.QUERY_CHUNK))
        with torch.no_grad():
            chunks = self._pair_chunks()
            for q0 in range(0, nq, qchunk):
                q1 = min(nq, q0 + qchunk)
                pos = positions[q0:q1]
                Gp = global_scores[q0:q1].to(dev) if global_scores is not None else self._pair_globals(features[q0:q1], pos.long())
                ops.maxsim_pair_scores(tokens[q0:q1], chunks, self._chunk, pos, Gp, self.alpha, self.scale, gallery_is_image,
                                       out=scores[q0:q1])
            if k is None:
                return scores
            best_val, best_idx = ops.topk_init(nq, k, dev)
            if nq == 0 or C == 0:
                return best_val, best_idx.to(torch.int64)
            # columns in the order of their gallery positions: the merge kernel's tie rule (smaller column) is then the index's
            by_pos, order = torch.sort(positions.long(), dim=1, stable=True)
            ops.topk_merge(scores.gather(1, order), 0, 0, best_val, best_idx)
            pos = by_pos.gather(1, best_idx.long().clamp_(min=0))
            pos = torch.where(best_idx >= 0, pos, torch.full_like(pos, -1))
        return best_val, self._ids_of(pos)

    def _ids_of(self, pos):
        """gallery positions [.., k] int64 (-1 = none) -> ids"""
        if self._running_ids:
            return pos
        found = self._ids[:self._n][pos.clamp(min=0)]
        return torch.where(pos >= 0, found, torch.full_like(found, -1))

    def _search_two_stage(self, features, tokens, k, C):
        self._refuse_rerank("search(candidates=C)")
        if not 1 <= k <= C <= ops.TOPK_MAX_K:
            raise ValueError(f"LateInteractionIndex.search: candidates must satisfy k <= C <= {ops.TOPK_MAX_K} (got k = {k}, C = {C})")
        if tokens is None or not self._tok and self._n:
            raise ValueError("LateInteractionIndex.search: alpha != 1 needs token features on both sides")
        nq = features.shape[0]
        dev = self.device
        features = features.detach().to(dev).float().contiguous()
        cand_val, cand_idx = ops.topk_init(nq, C, dev)
        if nq == 0 or self._n == 0:
            best_val, best_idx = ops.topk_init(nq, k, dev)
            return best_val, best_idx.to(torch.int64)
        gallery_is_image = self.kind == "image"
        qchunk = min(max(1, int(self.QUERY_CHUNK)), nq)
        from .train import similarity_matrix
        with torch.no_grad():
            for q0 in range(0, nq, qchunk):                      # stage 1: the C best by the global similarity
                q1 = min(nq, q0 + qchunk)
                for base, gf, _ in self.chunks():
                    G = similarity_matrix(gf, features[q0:q1]) if gallery_is_image else similarity_matrix(features[q0:q1], gf)
                    ops.topk_merge(G, 1 if gallery_is_image else 0, base, cand_val[q0:q1], cand_idx[q0:q1])
        return self.rerank(features, tokens, cand_idx, k, global_scores=cand_val)     # stage 2

    # ------------------------------------------------------------------ through a model
    @classmethod
    def from_model(cls, model, kind, alpha=None, device=None, token_dtype=None):
        """An empty index scored like `model`: a ColXLIP model gives alpha (default: the model's) and logit_scale.exp(); a plain
        CLIP model scores on its global features alone (alpha = 1, the scale applied to the image features as in its
        get_logits)."""
        from .model import ColXLIP
        from .train import unwrap_model
        core = unwrap_model(model)
        late = isinstance(core, ColXLIP)
        if not late and alpha is not None and float(alpha) != 1.0:
            raise ValueError("LateInteractionIndex.from_model: a model without token features scores with alpha = 1")
        alpha = (core.alpha if alpha is None else float(alpha)) if late else 1.0
        device = device or core.logit_scale.device
        return cls(kind, alpha=alpha, scale=float(core.logit_scale.detach().exp()), device=device, prescale=not late,
                   token_dtype=token_dtype)

    @staticmethod
    def _encode(model, what, batch):
        from .train import unwrap_model
        core = unwrap_model(model)
        with torch.no_grad():
            out = (core.encode_image if what == "image" else core.encode_text)(batch, normalize=True)
        if isinstance(out, tuple):
            return out[0].float(), out[1]
        return out.float(), None

    def _add_encoded(self, model, what, batch, ids):
        if self.kind != what:
            raise ValueError(f"LateInteractionIndex: this index holds {self.kind}s")
        return self.add(*self._encode(model, what, batch), ids=ids)

    def _search_encoded(self, model, what, batch, k, candidates=None):
        if self.kind == what:
            raise ValueError(f"LateInteractionIndex: an index of {self.kind}s is queried with the other side")
        return self.search(*self._encode(model, what, batch), k, candidates=candidates)

    def add_images(self, model, images, ids=None):
        return self._add_encoded(model, "image", images, ids)

    def add_texts(self, model, texts, ids=None):
        return self._add_encoded(model, "text", texts, ids)

    def search_texts(self, model, texts, k, candidates=None):
        return self._search_encoded(model, "text", texts, k, candidates)

    def search_images(self, model, images, k, candidates=None):
        return self._search_encoded(model, "image", images, k, candidates)

    # ------------------------------------------------------------------ files
    def save(self, path):
        """meta.json + features.npy [n, E] fp32 + tokens.npy [n, q, E] (bf16 as uint16 bit patterns; absent without tokens) +
        ids.npy [n] int64, written chunk by chunk.  An fp8 index: tokens.npy holds the e4m3 bytes (uint8), token_exp.npy [n, q]
        int32 the exponents, token_cnt.npy [n] int32 (text gallery) the packed rows per caption; meta token_dtype = "e4m3"."""
        os.makedirs(path, exist_ok=True)
        e = self._feat[0].shape[1] if self._feat else 0
        meta = {"kind": self.kind, "alpha": self.alpha, "scale": self.scale, "prescale": self.prescale, "n": self._n,
                "embed_dim": e, "tokens": None, "token_dtype": None, "chunk_items": self._chunk}
        feats = np.lib.format.open_memmap(os.path.join(path, "features.npy"), mode="w+", dtype=np.float32, shape=(self._n, e))
        toks, side = None, []
        fp8 = self.token_dtype == "fp8" and bool(self._tok)
        if self._tok:
            probe, name = _to_numpy(self._tok[0][:0])
            meta["tokens"], meta["token_dtype"] = list(self._tok[0].shape[1:]), "e4m3" if fp8 else name
            toks = np.lib.format.open_memmap(os.path.join(path, "tokens.npy"), mode="w+", dtype=probe.dtype,
                                             shape=(self._n,) + tuple(self._tok[0].shape[1:]))
        elif os.path.exists(os.path.join(path, "tokens.npy")):
            os.remove(os.path.join(path, "tokens.npy"))
        for name, store in zip(_FP8_FILES, (self._tok_exp, self._tok_cnt)):
            if fp8 and store:
                side.append(np.lib.format.open_memmap(os.path.join(path, name), mode="w+", dtype=np.int32,
                                                      shape=(self._n,) + tuple(store[0].shape[1:])))
            elif os.path.exists(os.path.join(path, name)):
                os.remove(os.path.join(path, name))
        for base, gf, gt in self.chunks():
            feats[base:base + gf.shape[0]] = gf.cpu().numpy()
            if fp8:
                gt, *rest = gt
                for arr, x in zip(side, rest):
                    arr[base:base + gf.shape[0]] = x.cpu().numpy()
            if toks is not None:
                toks[base:base + gf.shape[0]] = _to_numpy(gt)[0]
        feats.flush()
        for arr in side + ([toks] if toks is not None else []):
            arr.flush()
        np.save(os.path.join(path, "ids.npy"), self.ids.cpu().numpy())
        with open(os.path.join(path, "meta.json"), "w") as f:
            json.dump(meta, f, indent=1)
        return path

    @classmethod
    def load(cls, path, device="cuda"):
        """The index `save` wrote: the arrays are memory-mapped and copied to `device` `IO_ITEMS` items at a time."""
        with open(os.path.join(path, "meta.json")) as f:
            meta = json.load(f)
        fp8 = meta.get("token_dtype") == "e4m3"
        index = cls(meta["kind"], alpha=meta["alpha"], scale=meta["scale"], device=device, prescale=meta.get("prescale", False),
                    token_dtype="fp8" if fp8 else None)
        n = int(meta["n"])
        feats = np.load(os.path.join(path, "features.npy"), mmap_mode="r")
        toks = np.load(os.path.join(path, "tokens.npy"), mmap_mode="r") if meta["tokens"] is not None else None
        ids = np.load(os.path.join(path, "ids.npy"), mmap_mode="r")
        side = []                                    # an fp8 index: the exponents and (text gallery) the counts, kept as saved
        if fp8:
            side = [np.load(os.path.join(path, name), mmap_mode="r") for name in _FP8_FILES[:2 if meta["kind"] == "text" else 1]]
        if feats.shape[0] != n or ids.shape[0] != n or any(a.shape[0] != n for a in side + ([toks] if toks is not None else [])):
            raise ValueError(f"{path}: the arrays do not hold the {n} items meta.json names")
        running = bool(n == 0 or np.array_equal(ids, np.arange(n, dtype=np.int64)))
        step = max(1, int(cls.IO_ITEMS))
        for lo in range(0, n, step):
            hi = min(n, lo + step)
            if toks is None:
                tok = None
            elif fp8:
                tok = (_from_numpy(toks[lo:hi], "uint8"),) + tuple(_from_numpy(a[lo:hi], "int32") for a in side)
            else:
                tok = _from_numpy(toks[lo:hi], meta["token_dtype"])
            index.add(_from_numpy(feats[lo:hi], "float32"), tok, ids=torch.from_numpy(np.array(ids[lo:hi])))
        index._running_ids = running
        return index


# ---------------------------------------------------------------------------------------------------- command line
def build_parser():
    from .params import build_parser as train_parser
    parser = train_parser()
    parser.description = "index one side of a retrieval split and search it with the other"
    parser.add_argument("--direction", choices=["t2i", "i2t"], default="t2i",
                        help="t2i: text queries over the images; i2t: image queries over the captions")
    parser.add_argument("--k", type=int, default=10)
    parser.add_argument("--out", type=str, default=None, help="results.npz: scores, ids, query_ids")
    parser.add_argument("--save-index", type=str, default=None)
    parser.add_argument("--load-index", type=str, default=None)
    parser.add_argument("--index-dtype", choices=["model", "fp8"], default="model",
                        help="token storage of a new index: the model's compute dtype, or e4m3 bytes + one exponent per token "
                             "(half the bytes, scored on the fp8 MFMA); --load-index takes it from the saved meta.json")
    parser.add_argument("--candidates", type=int, default=0,
                        help="0: score every gallery item (exhaustive).  C >= --k: two stages, the C best items per query by the "
                             "global similarity, then the full late-interaction score of those only")
    return parser


def parse_args(argv):
    args = build_parser().parse_args(argv)
    if args.save_index and args.load_index:
        raise SystemExit("--save-index and --load-index exclude each other")
    if not 1 <= args.k <= ops.TOPK_MAX_K:
        raise SystemExit(f"--k must be in 1 .. {ops.TOPK_MAX_K}")
    if args.candidates:
        if not args.k <= args.candidates <= ops.TOPK_MAX_K:
            raise SystemExit(f"--candidates must be 0 (exhaustive) or in --k .. {ops.TOPK_MAX_K}")
        if args.index_dtype == "fp8":
            raise SystemExit("--candidates reranks bf16 / fp32 tokens; it excludes --index-dtype fp8")
        if getattr(args, "evaluate_as_original_clip", False):
            raise SystemExit("--candidates excludes --evaluate-as-original-clip: with alpha = 1 the exact search is already the global one")
    return args


def recall_at(ids, query_ids, truth, ks=(1, 5, 10)):
    """{K: share of queries with one of their true items among the first K returned ids}; `truth`: query id -> gallery id or
    list of gallery ids.  Only K <= the number of returned columns."""
    ids = np.asarray(ids)
    hits = np.zeros(ids.shape, dtype=bool)
    for row, qid in enumerate(np.asarray(query_ids).tolist()):
        want = truth[int(qid)]
        want = list(want) if isinstance(want, (list, tuple)) else [want]
        hits[row] = np.isin(ids[row], np.asarray(want, dtype=np.int64))
    return {K: float(hits[:, :K].any(axis=1).mean()) for K in ks if K <= ids.shape[1]}


def run(args):
    from .data import get_data
    from .factory import create_model_and_transforms
    from .model import ColXLIP, get_input_dtype
    from .train import RETRIEVAL_SPLITS
    args.rank, args.local_rank, args.world_size, args.distributed = 0, 0, 1, False
    device = torch.device(args.device)
    torch.manual_seed(args.seed)
    model, pre_train, pre_val = create_model_and_transforms(
        args.model, args.pretrained, precision=args.precision, device=device, force_quick_gelu=args.force_quick_gelu,
        force_patch_dropout=args.force_patch_dropout, force_image_size=args.force_image_size, output_dict=True)
    model.eval()
    data = get_data(args, (pre_train, pre_val), model=model)
    split = next((s for s in RETRIEVAL_SPLITS if s in data), None)
    if split is None:
        raise SystemExit("no retrieval split: pass --retrieval-coco or --retrieval-flickr")
    txt_data, img_data, img2txt_dict, txt2img_dict = data[split]
    input_dtype = get_input_dtype(args.precision)

    def images():
        for batch, ids in img_data.dataloader:
            yield batch.to(device=device, dtype=input_dtype, non_blocking=True), torch.as_tensor(ids).reshape(-1).cpu()

    def texts():
        for batch, ids in txt_data.dataloader:
            batch = batch.to(device=device, non_blocking=True)
            yield (batch[:, 0] if batch.ndim == 3 else batch).contiguous(), torch.as_tensor(ids).reshape(-1).cpu()

    t2i = args.direction == "t2i"
    gallery, queries = (images, texts) if t2i else (texts, images)
    kind, other = ("image", "text") if t2i else ("text", "image")
    if args.load_index:
        index = LateInteractionIndex.load(args.load_index, device)
        if index.kind != kind:
            raise SystemExit(f"{args.load_index} holds {index.kind}s; --direction {args.direction} needs {kind}s")
    else:
        alpha = None
        if isinstance(model, ColXLIP):
            alpha = 1.0 if getattr(args, "evaluate_as_original_clip", False) else float(args.alpha)
        index = LateInteractionIndex.from_model(model, kind, alpha=alpha, device=device,
                                                token_dtype="fp8" if args.index_dtype == "fp8" else None)
        for batch, ids in gallery():
            index._add_encoded(model, kind, batch, ids)
        if args.save_index:
            index.save(args.save_index)
    scores, found, query_ids = [], [], []
    for batch, ids in queries():
        s, i = index._search_encoded(model, other, batch, args.k, candidates=args.candidates or None)
        scores.append(s)
        found.append(i)
        query_ids.append(ids)
    scores, found, query_ids = torch.cat(scores).cpu().numpy(), torch.cat(found).cpu().numpy(), torch.cat(query_ids).numpy()
    truth = {int(c): [int(i) for i in (v if isinstance(v, (list, tuple)) else [v])] for c, v in
             (txt2img_dict if t2i else img2txt_dict).items()}
    name = "text_to_image" if t2i else "image_to_text"
    metrics = {f"{name}_R@{K}": v for K, v in recall_at(found, query_ids, truth).items()}
    logging.info(f"Search {split} {args.direction}: {len(query_ids)} queries over {len(index)} {kind}s, k = {args.k}\t" +
                 "\t".join(f"{m}: {v:.4f}" for m, v in metrics.items()))
    if args.out:
        np.savez(args.out, scores=scores, ids=found, query_ids=query_ids,
                 metric_names=np.array(list(metrics)), metric_values=np.array(list(metrics.values()), dtype=np.float64))
    return metrics


def main(argv=None):
    import sys
    logging.basicConfig(level=logging.INFO, format="%(asctime)s | %(levelname)s | %(message)s")
    run(parse_args(sys.argv[1:] if argv is None else argv))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
