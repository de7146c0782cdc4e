"""Epoch driver for the CLIP train step (boundary: reference train.py:93-270 `train_one_epoch`, called from
main.py:413; only the call signature, the accumulation semantics of train.py:138-185 and the format of the
"Train Epoch" log line -- the in-band source of the samples/s metric, train.py:236-262 -- are kept; the body is this
stack's own).

One optimizer step = collect `accum_freq` micro-batches -> forward/backward (plain, or the two-pass feature-caching
scheme when accumulating) -> gradient mean across ranks (GradSync; nothing to do when the model is DDP-wrapped, the
engines' hooks already reduced inside the backward) -> optional global-norm clip -> fused AdamW -> logit_scale clamp.
Precision lives inside the model (bf16 operands, fp32 masters): no autocast.  A torch GradScaler is honoured when
one is passed (the reference creates one for `--precision amp`), but none is needed for bf16."""
import logging
import math
import time

import torch

from . import ops
from .distributed import is_master
from .model import get_input_dtype
from .optim import clip_grad_norm_, sharded_clip_grad_norm_

LOGIT_SCALE_MAX = math.log(100)       # the CLIP paper's clamp, reference train.py:211-212


class AverageMeter:
    """Last value and running mean of a series (name used by the reference's callers)."""

    __slots__ = ("val", "sum", "count")

    def __init__(self):
        self.reset()

    def reset(self):
        self.val, self.sum, self.count = 0.0, 0.0, 0

    def update(self, val, n=1):
        self.val = val
        self.sum += val * n
        self.count += n

    @property
    def avg(self):
        return self.sum / self.count if self.count else 0.0


def unwrap_model(model):
    return getattr(model, "module", model)


def _with_total(losses):
    """The loss dict's sum is its total when it names none, as in open_clip's trainer: SigLipLoss returns only
    `contrastive_loss` (reference loss.py:604), DistillClipLoss `contrastive_loss` and `distill_loss` (loss.py:375), while
    the loop reads `total_loss` (reference train.py:135)."""
    if "total_loss" not in losses:
        losses["total_loss"] = sum(losses.values())
    return losses


def backward(total_loss, scaler=None):
    (scaler.scale(total_loss) if scaler is not None else total_loss).backward()


class _StepRunner:
    """Everything between 'a full group of micro-batches is on the device' and 'the weights have moved'."""

    def __init__(self, model, loss, optimizer, scaler, args, grad_sync, dist_model=None):
        self.model, self.loss, self.optimizer, self.scaler, self.args, self.grad_sync = model, loss, optimizer, scaler, args, grad_sync
        self.dist_model = dist_model
        self.clip = getattr(args, "grad_clip_norm", None)

    def _no_sync(self):
        gs = self.grad_sync
        if gs is not None:
            return gs.no_sync()
        if hasattr(self.model, "no_sync"):            # DistributedDataParallel
            return self.model.no_sync()
        import contextlib
        return contextlib.nullcontext()

    def _single(self, images, texts):
        dist_out = None
        if self.dist_model is not None:
            # the teacher (open_clip trainer semantics): no graph, so the towers keep no activations; its outputs enter the
            # loss as dist_image_features / dist_text_features / dist_logit_scale
            with torch.no_grad():
                dist_out = self.dist_model(images, texts)
        out = self.model(images, texts)
        if dist_out is not None:
            out.update({f"dist_{k}": v for k, v in dist_out.items()})
        logit_scale = out["logit_scale"]
        losses = _with_total(self.loss(**out, output_dict=True))
        backward(losses["total_loss"], self.scaler)
        return losses, logit_scale

    def _accumulated(self, group):
        """reference train.py:138-185: features of every micro-batch are first computed without a graph; then each
        micro-batch is re-run with a graph and the loss is taken over ALL features with that micro-batch's fresh ones
        spliced in at its position, so every sample sees the full set of negatives."""
        cached = {}
        with torch.no_grad():
            for images, texts in group:
                out = self.model(images, texts)
                for key, val in out.items():
                    if key not in ("logit_scale", "logit_bias"):
                        cached.setdefault(key, []).append(val)
        losses = logit_scale = None
        last = len(group) - 1
        for j, (images, texts) in enumerate(group):
            ctx = self._no_sync() if j < last else _null()
            with ctx:            # only the last backward needs the cross-rank mean of the accumulated gradients
                out = self.model(images, texts)
                scalars = {k: out.pop(k) for k in ("logit_scale", "logit_bias") if k in out}
                logit_scale = scalars["logit_scale"]
                feats = {key: torch.cat(vals[:j] + [out[key]] + vals[j + 1:]) for key, vals in cached.items()}
                losses = _with_total(self.loss(**feats, **scalars, output_dict=True))
                backward(losses["total_loss"], self.scaler)
        return losses, logit_scale

    def __call__(self, group):
        self.optimizer.zero_grad()
        if len(group) == 1:
            losses, logit_scale = self._single(*group[0])
        else:
            losses, logit_scale = self._accumulated(group)
        if self.grad_sync is not None:
            self.grad_sync.sync()
            self.grad_sync.wait()
        params = [p for p in self.model.parameters() if p.grad is not None]
        if self.clip is not None and getattr(self.grad_sync, "shard", False):      # reduce-scattered gradients: norm over the slices
            assert self.scaler is None, "--shard-optimizer with a GradScaler is not supported"
            sharded_clip_grad_norm_(self.grad_sync, params, self.clip)
            self.optimizer.step()
        elif self.scaler is not None:
            if self.clip is not None:
                self.scaler.unscale_(self.optimizer)
                clip_grad_norm_(params, self.clip)
            self.scaler.step(self.optimizer)
            self.scaler.update()
        else:
            if self.clip is not None:
                clip_grad_norm_(params, self.clip)
            self.optimizer.step()
        with torch.no_grad():
            ops.clamp1(unwrap_model(self.model).logit_scale.data, 0.0, LOGIT_SCALE_MAX)
        return losses, logit_scale


class _null:
    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False


def train_one_epoch(model, data, loss, epoch, optimizer, scaler, scheduler, dist_model, args, tb_writer=None,
                    grad_sync=None):
    device = torch.device(args.device)
    input_dtype = get_input_dtype(args.precision)
    accum = max(1, int(args.accum_freq))
    model.train()
    if dist_model is not None:
        assert accum == 1, "distillation does not support --accum-freq > 1"
        dist_model.eval()
    info = data["train"]
    info.set_epoch(epoch)
    loader = info.dataloader
    steps_per_epoch = loader.num_batches // accum
    digits = math.ceil(math.log(loader.num_samples + 1, 10))
    run_step = _StepRunner(model, loss, optimizer, scaler, args, grad_sync, dist_model)

    def logs_at(step_in_epoch):
        return step_in_epoch % args.log_every_n_steps == 0 or step_in_epoch + 1 == steps_per_epoch

    meters = {}
    batch_time, data_time = AverageMeter(), AverageMeter()
    group = []
    mark = time.time()
    for i, (images, texts) in enumerate(loader):
        if i // accum >= steps_per_epoch:
            break                                   # a trailing partial group never makes a step
        images = images.to(device=device, dtype=input_dtype, non_blocking=True)
        texts = texts[:, 0].to(device=device, non_blocking=True).contiguous()      # first caption (train.py:121-122)
        group.append((images, texts))
        if len(group) < accum:
            continue
        done = i // accum                            # optimizer steps finished so far in this epoch
        if not args.skip_scheduler:
            scheduler(steps_per_epoch * epoch + done)
        data_time.update(time.time() - mark)
        losses, logit_scale = run_step(group)
        per_gpu = len(group[-1][0])
        group = []
        if device.type == "cuda" and (logs_at(done) or logs_at(done + 1)):
            # the step time a log line reports must be device time, not launch time: drain the queue at both ends of
            # a logged step (the reference's loop only drains at its .item() calls)
            torch.cuda.synchronize(device)
        batch_time.update(time.time() - mark)
        mark = time.time()
        done += 1
        if is_master(args) and logs_at(done - 1):
            for key, val in losses.items():
                meters.setdefault(key, AverageMeter()).update(val.item(), per_gpu)
            seen = done * per_gpu * accum * args.world_size
            rate = accum * args.batch_size * args.world_size / batch_time.val
            rate_gpu = accum * args.batch_size / batch_time.val
            loss_log = " ".join(f"{name.capitalize()}: {m.val:#.5g} ({m.avg:#.5g})" for name, m in meters.items())
            logging.info(
                f"Train Epoch: {epoch} [{seen:>{digits}}/{loader.num_samples} ({100.0 * done / steps_per_epoch:.0f}%)] "
                f"Data (t): {data_time.avg:.3f} "
                f"Batch (t): {batch_time.avg:.3f}, {rate:#g}/s, {rate_gpu:#g}/s/gpu "
                f"LR: {optimizer.param_groups[0]['lr']:5f} "
                f"Logit Scale: {math.log(logit_scale.item()):.3f} " + loss_log
            )
            if tb_writer is not None:
                step = steps_per_epoch * epoch + done - 1
                for name, m in meters.items():
                    tb_writer.add_scalar("train/" + name, m.val, step)
                tb_writer.add_scalar("train/samples_per_second", rate, step)
            batch_time.reset()
            data_time.reset()
    return meters


# --------------------------------------------------------------------------- evaluation
# keys under which the reference's get_data stores a retrieval split (train.py:286-343); each value is
# (text DataInfo, image DataInfo, img2txt_dict, txt2img_dict)
RETRIEVAL_SPLITS = ("retrieval_coco", "retrieval_flickr", "retrieval_cc3m_train", "retrieval_docci", "retrieval_urban_1k",
                    "retrieval_iiw", "retrieval_dci", "retrieval_sharegpt4v-1k", "retrieval_sharegpt4v-10k")


def evaluate(model, data, epoch, args, tb_writer=None, tokenizer=None):
    """Boundary: reference train.py:273-376 (called from main.py:396,411).  Master rank only; for every retrieval split
    present in `data`, at the reference's cadence (`--val-frequency`, and always after the last epoch), both towers encode
    their side in batches ON the GPU, the similarity matrix is one fp32 GEMM, ranks come from `clipx_retrieval_rank`; the
    metric names, the "Eval Epoch" log line and `results.jsonl` are the reference's.  Zero-shot classification sets
    (`imagenet-val`, `imagenet-v2`; open_clip_train.zero_shot) and FLAIR inference are outside this stack."""
    import json
    import os
    metrics = {}
    if not is_master(args):
        return metrics
    if any(k in data for k in ("imagenet-val", "imagenet-v2")):
        raise NotImplementedError("zero-shot classification eval (open_clip_train.zero_shot) is outside the MI355X hot path")
    if getattr(args, "inference_with_flair", False):
        raise NotImplementedError("--inference-with-flair (text-conditioned attention pooling) is outside the MI355X hot path")
    device = torch.device(args.device)
    was_training = model.training
    model.eval()
    input_dtype = get_input_dtype(args.precision)
    if args.val_frequency and ((epoch % args.val_frequency) == 0 or epoch == args.epochs):
        for split in RETRIEVAL_SPLITS:
            if split in data:
                txt_data, img_data, img2txt_dict, txt2img_dict = data[split]
                metrics = retrieval_on_split(split, model, txt_data.dataloader, img_data.dataloader, img2txt_dict,
                                             txt2img_dict, args, epoch, metrics, device, input_dtype)
    model.train(was_training)
    if not metrics:
        return metrics
    logging.info(f"Eval Epoch: {epoch} " + "\t".join(f"{k}: {round(v, 4):.4f}" for k, v in metrics.items()))
    if getattr(args, "save_logs", False):
        if tb_writer is not None:
            for name, val in metrics.items():
                tb_writer.add_scalar("val/" + name, val, epoch)
        with open(os.path.join(args.checkpoint_path, "results.jsonl"), "a+") as f:
            f.write(json.dumps(metrics) + "\n")
    return metrics


def encode_split(model, txt_loader, img_loader, device, input_dtype=None, with_tokens=False):
    """(image_features [n_img, E], image ids, text_features [n_txt, E], caption ids): every batch of the two loaders through
    `encode_text` / `encode_image(normalize=True)` without a graph; features stay on the device (the reference moves every
    batch to the CPU and encodes images one at a time, train.py:520-541,590-606).  A model whose encoders return (pooled,
    tokens) pairs (ColXLIP) contributes its pooled features here; with `with_tokens` the normalised token features, on the
    device in the model's compute dtype, follow as a fifth and sixth value ([n_img, q, E], [n_txt, n, E])."""
    core = unwrap_model(model)
    feats_t, ids_t, feats_i, ids_i, toks_t, toks_i = [], [], [], [], [], []

    def keep(out, feats, toks):
        if isinstance(out, tuple):
            if with_tokens:
                toks.append(out[1])
            out = out[0]
        feats.append(out.float())

    with torch.no_grad():
        for texts, cap_id in txt_loader:
            texts = texts.to(device=device, non_blocking=True)
            if texts.ndim == 3:
                texts = texts[:, 0]
            keep(core.encode_text(texts.contiguous(), normalize=True), feats_t, toks_t)
            ids_t.append(torch.as_tensor(cap_id).reshape(-1).cpu())
        for images, img_id in img_loader:
            images = images.to(device=device, dtype=input_dtype, non_blocking=True)
            keep(core.encode_image(images, normalize=True), feats_i, toks_i)
            ids_i.append(torch.as_tensor(img_id).reshape(-1).cpu())
    found = (torch.cat(feats_i), torch.cat(ids_i), torch.cat(feats_t), torch.cat(ids_t))
    if with_tokens:
        if not toks_i or not toks_t:
            raise ValueError("encode_split(with_tokens=True): the model's encoders return no token features")
        found += (torch.cat(toks_i), torch.cat(toks_t))
    return found


def is_late_interaction(model) -> bool:
    """a model that scores with alpha * global + (1 - alpha) * token MaxSim (ColXLIP)"""
    from .model import ColXLIP
    return isinstance(unwrap_model(model), ColXLIP)


def late_interaction_scores(model, txt_loader, img_loader, device, input_dtype=None, alpha=0.5):
    """(scores [n_img, n_txt] fp32, image ids, caption ids) of a ColXLIP model on one retrieval split:
    logit_scale.exp() * (alpha * I T^T + (1 - alpha) * MaxSim(tokens)^T) -- the scoring the reference's ColXLIP.forward carries
    as a commented-out block (model.py:670-685) -- on `ops.maxsim_scores`.  alpha = 1 is the reference's `original_clip` mode:
    the token features are then not even collected."""
    tokens = alpha != 1.0
    found = encode_split(model, txt_loader, img_loader, device, input_dtype, with_tokens=tokens)
    feats_i, img_ids, feats_t, cap_ids = found[:4]
    with torch.no_grad():
        scale = float(unwrap_model(model).logit_scale.exp())
        G = similarity_matrix(feats_i, feats_t)
        scores = ops.maxsim_scores(found[4], found[5], G, alpha, scale) if tokens else ops.maxsim_scores(None, None, G, 1.0, scale)
    return scores, img_ids, cap_ids


def remap_indices(img_ids, cap_ids, img2txt_dict, txt2img_dict):
    """Dataset image ids -> row index of the image in the encoded matrix (reference train.py:429-454).  Caption ids must
    already be the row indices of the text matrix, which is what the reference assumes too."""
    row_of = {int(old): row for row, old in enumerate(img_ids.tolist())}
    if cap_ids.tolist() != list(range(len(cap_ids))):
        raise ValueError("retrieval split: caption ids must enumerate the text loader's rows in order")
    img2txt = {row_of[int(i)]: list(caps) for i, caps in img2txt_dict.items()}
    txt2img = {int(c): row_of[int(imgs[0] if isinstance(imgs, (list, tuple)) else imgs)] for c, imgs in txt2img_dict.items()}
    return img2txt, txt2img


def retrieval_on_split(keyword, model, txt_loader, img_loader, img2txt_dict, txt2img_dict, args, epoch, metrics, device,
                       input_dtype=None, autocast=None):
    """reference train.py:510-587 (`original_clip` mode).  A ColXLIP model is scored by late interaction with `args.alpha`
    (`late_interaction_scores`), or on its global features alone under --evaluate-as-original-clip; the ranking and the metric
    names are the same.  `autocast` is accepted for signature compatibility and unused: precision lives inside the model."""
    if is_late_interaction(model):
        alpha = 1.0 if getattr(args, "evaluate_as_original_clip", False) else float(getattr(args, "alpha", 0.5))
        scores, img_ids, cap_ids = late_interaction_scores(model, txt_loader, img_loader, device, input_dtype, alpha)
    else:
        feats_i, img_ids, feats_t, cap_ids = encode_split(model, txt_loader, img_loader, device, input_dtype)
        with torch.no_grad():
            scale = unwrap_model(model).logit_scale.exp().float()
            scores = similarity_matrix(feats_i * scale, feats_t)              # [n_img, n_txt], as train.py:608
    img2txt, txt2img = remap_indices(img_ids, cap_ids, img2txt_dict, txt2img_dict)
    found = compute_retrieval(scores, txt2img, img2txt)
    prefix = keyword + "_" if keyword else ""
    metrics.update({prefix + k: v for k, v in found.items()})
    metrics.setdefault("epoch", epoch)
    metrics[prefix + "num_text_samples"] = txt_loader.num_samples
    metrics[prefix + "num_image_samples"] = img_loader.num_samples
    return metrics


def similarity_matrix(image_features, text_features):
    """image_features @ text_features.T in fp32 on the HIP GEMM (reference train.py computes it with torch matmul)."""
    import torch
    from . import ops
    a = image_features.contiguous().float()
    b = text_features.contiguous().float()
    r, e = a.shape
    c = b.shape[0]
    z = torch.empty((r, c), dtype=torch.float32, device=a.device)
    ops.gemm_f32(r, c, e, a, e, 1, b, 1, e, z, c)
    return z


def compute_retrieval(similarity_scores, txt2img, img2txt):
    """reference train.py:457-508 with the per-row CPU argsort + search replaced by a rank-count kernel on the GPU.
    similarity_scores: [n_img, n_txt] (or a tuple (i2t [n_img, n_txt], t2i [n_txt, n_img])); txt2img: caption index ->
    image index; img2txt: image index -> list of caption indices.  Returns the reference's metric names.  A rank is the
    number of candidates scoring strictly higher (identical to the argsort position unless scores tie exactly)."""
    import numpy as np
    import torch
    from . import ops
    if isinstance(similarity_scores, tuple):
        i2t, t2i = similarity_scores
    else:
        i2t, t2i = similarity_scores, similarity_scores.t()
    i2t = i2t.float()
    t2i = t2i.float().contiguous()                       # rows = captions
    if i2t.stride(1) != 1:
        i2t = i2t.contiguous()
    dev = i2t.device
    n_txt, n_img = t2i.shape
    t_off = torch.arange(n_txt + 1, dtype=torch.int32, device=dev)
    t_idx = torch.tensor([int(txt2img[i]) for i in range(n_txt)], dtype=torch.int32, device=dev)
    t2i_ranks = ops.retrieval_rank(t2i, t_off, t_idx).float().cpu()
    lens = [len(img2txt[i]) for i in range(n_img)]
    i_off = torch.tensor(np.concatenate([[0], np.cumsum(lens)]), dtype=torch.int32, device=dev)
    i_idx = torch.tensor([int(c) for i in range(n_img) for c in img2txt[i]], dtype=torch.int32, device=dev)
    i2t_ranks = ops.retrieval_rank(i2t, i_off, i_idx).float().cpu()

    def report(prefix, ranks):
        n = len(ranks)
        return {
            f"{prefix}_R@1": float((ranks < 1).sum()) / n,
            f"{prefix}_R@5": float((ranks < 5).sum()) / n,
            f"{prefix}_R@10": float((ranks < 10).sum()) / n,
            f"{prefix}_mean_rank": ranks.mean().item() + 1,
            f"{prefix}_median_rank": float(np.floor(np.median(ranks.numpy())) + 1),     # a Python float: results.jsonl is JSON
        }

    return {**report("text_to_image", t2i_ranks), **report("image_to_text", i2t_ranks)}
