"""Public factory API with the reference's signatures (reference factory.py:35-461).

Only the plain-CLIP branch of `create_model` is on the MI355X hot path; branches that fetch
from the network (hf-hub, OpenAI / pretrained tags), timm / HF towers, torchscript and the
CoCa loss raise with a message saying so.
"""
import json
import logging
import math
import os
import re
from copy import deepcopy
from dataclasses import asdict, dataclass
from pathlib import Path
from typing import Any, Dict, Optional, Tuple, Union

import torch
import torch.nn.functional as F

from .loss import ClipLoss, ColClipLoss, DistillClipLoss, SigLipLoss
from .model import CLIP, ColXLIP, get_cast_dtype, set_model_preprocess_cfg

HF_HUB_PREFIX = 'hf-hub:'
_MODEL_CONFIG_PATHS = [Path(__file__).parent / "model_configs/"]

OPENAI_DATASET_MEAN = (0.48145466, 0.4578275, 0.40821073)
OPENAI_DATASET_STD = (0.26862954, 0.26130258, 0.27577711)


@dataclass
class PreprocessCfg:
    size: Union[int, Tuple[int, int]] = 224
    mode: str = 'RGB'
    mean: Tuple[float, ...] = OPENAI_DATASET_MEAN
    std: Tuple[float, ...] = OPENAI_DATASET_STD
    interpolation: str = 'bicubic'
    resize_mode: str = 'shortest'
    fill_color: int = 0


def merge_preprocess_dict(base, overlay: Dict):
    base = asdict(base) if isinstance(base, PreprocessCfg) else dict(base)
    for k, v in (overlay or {}).items():
        if k in base and v is not None:
            base[k] = v
    return base


def merge_preprocess_kwargs(base, **kwargs):
    return merge_preprocess_dict(base, kwargs) if base else {k: v for k, v in kwargs.items() if v is not None}


class TensorImageTransform:
    """Resize (bilinear/bicubic on the shortest side), centre crop and normalise a float
    [3,H,W] tensor in [0,1].  Stands in for the torchvision pipeline the reference builds with
    open_clip.transform.image_transform_v2 (torchvision/PIL decode is host-side, out of scope)."""

    def __init__(self, cfg: PreprocessCfg, is_train: bool):
        self.cfg, self.is_train = cfg, is_train

    def __call__(self, img: torch.Tensor) -> torch.Tensor:
        size = self.cfg.size if isinstance(self.cfg.size, (tuple, list)) else (self.cfg.size, self.cfg.size)
        img = img.float()
        if img.shape[-2:] != tuple(size):
            h, w = img.shape[-2:]
            s = max(size[0] / h, size[1] / w)
            nh, nw = max(size[0], round(h * s)), max(size[1], round(w * s))
            mode = 'bicubic' if self.cfg.interpolation == 'bicubic' else 'bilinear'
            img = F.interpolate(img[None], size=(nh, nw), mode=mode, align_corners=False)[0]
            top, left = (nh - size[0]) // 2, (nw - size[1]) // 2
            img = img[:, top:top + size[0], left:left + size[1]]
        mean = torch.tensor(self.cfg.mean, dtype=img.dtype, device=img.device).view(-1, 1, 1)
        std = torch.tensor(self.cfg.std, dtype=img.dtype, device=img.device).view(-1, 1, 1)
        return (img - mean) / std

    def __repr__(self):
        return f"TensorImageTransform(size={self.cfg.size}, train={self.is_train})"


class _ConfigRegistry:
    """name -> architecture dict, read from every `*.json` under the registered paths (a file or a directory each).
    A file counts as a model config when it names an embed_dim and both towers (the reference's rule,
    factory.py:62-68); names are listed in natural order (ViT-B-16 before ViT-B-32 before ViT-L-14)."""

    REQUIRED = ("embed_dim", "vision_cfg", "text_cfg")

    def __init__(self, *paths: Path):
        self.paths = list(paths)
        self.table: Dict[str, dict] = {}
        self.reload()

    @staticmethod
    def _order(name: str):
        return [int(tok) if tok.isdigit() else tok for tok in re.split(r"(\d+)", name.lower())]

    def _files(self):
        for root in self.paths:
            if root.is_dir():
                yield from sorted(root.glob("*.json"))
            elif root.suffix == ".json" and root.is_file():
                yield root

    def reload(self):
        found = dict(self.table)
        for path in self._files():
            cfg = json.loads(path.read_text())
            if all(key in cfg for key in self.REQUIRED):
                found[path.stem] = cfg
        self.table = {name: found[name] for name in sorted(found, key=self._order)}

    def add(self, path):
        self.paths.append(Path(path))
        self.reload()


_REGISTRY = _ConfigRegistry(*_MODEL_CONFIG_PATHS)


def list_models():
    """Architectures available by name (reference factory.py:77-79)."""
    return list(_REGISTRY.table)


def add_model_config(path):
    """Register one more config file or directory (reference factory.py:82-87)."""
    _MODEL_CONFIG_PATHS.append(Path(path))
    _REGISTRY.add(path)


def get_model_config(model_name):
    cfg = _REGISTRY.table.get(model_name)
    return deepcopy(cfg) if cfg is not None else None


class HashTokenizer:
    """Stand-in used ONLY when open_clip_torch (whose wheel carries CLIP's BPE vocabulary) is not installed: same call
    contract as its SimpleTokenizer -- `tok(str | list[str], context_length=None) -> LongTensor [n, context_length]`, rows
    `<start> ids... <end> 0...`, truncated rows still end in `<end>` (the id the text tower pools at) -- but ids are a CRC of
    each lower-cased whitespace-separated word, NOT byte-pair codes.  Good for synthetic runs and shape plumbing; a model
    trained or evaluated on real captions needs the real vocabulary."""

    def __init__(self, context_length: int = 77, vocab_size: int = 49408):
        self.context_length, self.vocab_size = context_length, vocab_size
        self.sot_token_id, self.eot_token_id = vocab_size - 2, vocab_size - 1

    def __call__(self, texts, context_length: Optional[int] = None) -> torch.Tensor:
        import zlib
        if isinstance(texts, str):
            texts = [texts]
        length = context_length or self.context_length
        out = torch.zeros(len(texts), length, dtype=torch.long)
        for row, text in enumerate(texts):
            ids = [1 + zlib.crc32(w.encode("utf-8")) % (self.vocab_size - 3) for w in text.lower().split()]
            ids = [self.sot_token_id] + ids[:length - 2] + [self.eot_token_id]
            out[row, :len(ids)] = torch.tensor(ids)
        return out


def get_tokenizer(model_name: str = '', context_length: Optional[int] = None, **kwargs):
    """reference factory.py:87-128.  open_clip_torch's tokenizer when that package is installed (its wheel holds the BPE
    vocabulary; nothing is downloaded here); otherwise a `HashTokenizer` with this model's context length and vocabulary
    size and a warning -- so the reference's unconditional `tokenizer = get_tokenizer(args.model)` (main.py:325) still
    returns a callable in a synthetic-data run."""
    try:
        from open_clip import get_tokenizer as _gt  # type: ignore
    except ImportError:
        cfg = get_model_config(_canonical_name(model_name)) or {}
        text_cfg = cfg.get("text_cfg", {})
        logging.warning("colxlip_amd.get_tokenizer: open_clip_torch is not installed, so CLIP's BPE vocabulary is not available; "
                        "returning HashTokenizer (word-hash ids: for synthetic data only)")
        return HashTokenizer(context_length or text_cfg.get("context_length", 77), text_cfg.get("vocab_size", 49408))
    return _gt(model_name, context_length=context_length, **kwargs)


def download_weights_from_hf(model_repo, filename):
    """Exported by the reference package (factory.py:35-44); needs the network."""
    raise RuntimeError("download_weights_from_hf needs network access; pass a local checkpoint path as `pretrained`")


def _strip_prefix(state_dict: dict, prefix: str) -> dict:
    n = len(prefix)
    return {(k[n:] if k.startswith(prefix) else k): v for k, v in state_dict.items()}


def load_state_dict(checkpoint_path: str, map_location='cpu'):
    """Tensors of a checkpoint file: a train checkpoint's `state_dict` entry or a bare state dict, with the `module.`
    prefix of a DistributedDataParallel-saved model removed (behaviour of reference factory.py:144-156).  The file is read
    with `weights_only=True`: nothing in it is executed."""
    blob = torch.load(checkpoint_path, map_location=map_location, weights_only=True)
    tensors = blob.get('state_dict', blob) if isinstance(blob, dict) else blob
    if tensors and all(k.startswith('module.') for k in tensors):
        tensors = _strip_prefix(tensors, 'module.')
    return tensors


def _resample(table: torch.Tensor, new_shape, mode: str, antialias: bool) -> torch.Tensor:
    """table [*old_shape, width] -> [*new_shape, width] by interpolating over the leading (position) axes."""
    nd = len(new_shape)
    chan_first = table.float().movedim(-1, 0).unsqueeze(0)                   # [1, width, *old_shape]
    out = F.interpolate(chan_first, size=tuple(new_shape), mode=mode, antialias=antialias, align_corners=False)
    return out.squeeze(0).movedim(0, nd)


def resize_pos_embed(state_dict, model, interpolation: str = 'bicubic', antialias: bool = True):
    """A checkpoint trained at another resolution: resample the patch-position grid of
    `visual.positional_embedding` to this model's grid; the class-token row is carried over unchanged
    (behaviour of reference model.py:355-388).  Host-side, once per load; edits `state_dict` in place."""
    key = 'visual.positional_embedding'
    table = state_dict.get(key)
    grid = getattr(model.visual, 'grid_size', None)
    if table is None or grid is None:
        return
    gh, gw = grid
    n_patch_old = table.shape[0] - 1
    if n_patch_old == gh * gw:
        return
    side = math.isqrt(n_patch_old)
    if side * side != n_patch_old:
        raise ValueError(f"{key}: {n_patch_old} patch positions do not form a square grid")
    logging.info('Resizing position embedding grid-size from %s to %s', (side, side), (gh, gw))
    cls_row, patches = table[:1], table[1:]
    patches = _resample(patches.reshape(side, side, -1), (gh, gw), interpolation, antialias)
    state_dict[key] = torch.cat([cls_row.float(), patches.reshape(gh * gw, -1)], dim=0)


def resize_text_pos_embed(state_dict, model, interpolation: str = 'linear', antialias: bool = False):
    """Same for the text tower's `positional_embedding` when the context length differs (reference model.py:391-418)."""
    key = 'positional_embedding'
    table = state_dict.get(key)
    target = getattr(model, key, None)
    if table is None or target is None:
        return
    assert table.shape[1] == target.shape[1], 'text pos_embed width changed!'
    if table.shape[0] == target.shape[0]:
        return
    logging.info('Resizing text position embedding num_pos from %s to %s', table.shape[0], target.shape[0])
    state_dict[key] = _resample(table, (target.shape[0],), interpolation, antialias)


def convert_to_custom_text_state_dict(state_dict: dict):
    """reference model.py:262-277: old flat text-tower keys -> `text.`-prefixed keys of CustomTextCLIP checkpoints."""
    if 'text_projection' in state_dict:
        new_state_dict = {}
        for k, v in state_dict.items():
            if any(k.startswith(p) for p in ('text_projection', 'positional_embedding', 'token_embedding', 'transformer',
                                             'ln_final')):
                k = 'text.' + k
            new_state_dict[k] = v
        return new_state_dict
    return state_dict


def _from_custom_text_state_dict(state_dict: dict):
    """The inverse direction, which is what THIS model needs: CustomTextCLIP-style checkpoints (`text.` prefix) loaded
    into the flat CLIP layout (reference model.py:285-309 keeps both layouts loadable)."""
    if any(k.startswith('text.') for k in state_dict) and 'text_projection' not in state_dict:
        return {(k[5:] if k.startswith('text.') else k): v for k, v in state_dict.items()}
    return state_dict


def load_checkpoint(model, checkpoint_path: str, strict: bool = True):
    """reference factory.py:159-201: `module.` prefix stripped, `text.`-prefixed checkpoints flattened, missing logit_bias
    filled, HF position_ids dropped, image / text position embeddings resized to the model, ColXLIP loaded non-strictly
    (a CLIP checkpoint has no token heads).  numpy big_vision checkpoints are outside this build."""
    if os.path.splitext(checkpoint_path)[1] in ('.npz', '.npy'):
        raise NotImplementedError("big_vision (SigLIP) numpy checkpoints are outside the MI355X hot path")
    state_dict = load_state_dict(checkpoint_path)
    state_dict = _from_custom_text_state_dict(state_dict)
    if 'logit_bias' not in state_dict and getattr(model, 'logit_bias', None) is not None:
        state_dict["logit_bias"] = torch.zeros_like(state_dict["logit_scale"])
    state_dict.pop('text.transformer.embeddings.position_ids', None)
    resize_pos_embed(state_dict, model)
    resize_text_pos_embed(state_dict, model)
    if isinstance(model, ColXLIP):
        strict = False
    return model.load_state_dict(state_dict, strict=strict)


def create_model(
        model_name: str,
        pretrained: Optional[str] = None,
        precision: str = 'fp32',
        device: Union[str, torch.device] = 'cpu',
        jit: bool = False,
        force_quick_gelu: bool = False,
        force_custom_text: bool = False,
        force_patch_dropout: Optional[float] = None,
        force_image_size: Optional[Union[int, Tuple[int, int]]] = None,
        force_preprocess_cfg: Optional[Dict[str, Any]] = None,
        pretrained_image: bool = False,
        pretrained_hf: bool = True,
        cache_dir: Optional[str] = None,
        output_dict: Optional[bool] = None,
        require_pretrained: bool = False,
        **model_kwargs,
):
    """reference factory.py:204-364, CLIP / ColXLIP branch.  Stages: resolve the architecture (name -> JSON config + the
    force_* overrides), refuse what this stack does not build, construct on `device` with fp32 master parameters (every
    precision; `precision` selects the kernels' operand type, see model.compute_dtype_for), optionally load a LOCAL
    checkpoint, attach the preprocess configuration."""
    device = torch.device(device) if isinstance(device, str) else device
    arch = _resolve_architecture(model_name, pretrained, force_quick_gelu, force_patch_dropout, force_image_size, model_kwargs)
    _refuse_unbuilt(arch, jit=jit, pretrained_image=pretrained_image, force_custom_text=force_custom_text)
    arch.pop('custom_text', None)
    name = _canonical_name(model_name)
    cls = ColXLIP if "colxlip" in name else CLIP            # reference factory.py:286-287
    model = cls(**arch, cast_dtype=get_cast_dtype(precision), precision=precision).to(device=device)

    loaded = False
    if pretrained:
        if not os.path.exists(pretrained):
            msg = (f'Pretrained weights ({pretrained}) not found for model {name}: only local checkpoint paths can be '
                   'loaded (pretrained tags need a download, there is no network path in this stack).')
            logging.warning(msg)
            raise RuntimeError(msg)
        logging.info(f'Loading pretrained {name} weights ({pretrained}).')
        load_checkpoint(model, pretrained, strict=False)
        loaded = True
    if require_pretrained and not loaded:
        raise RuntimeError(f'Pretrained weights were required for (model: {name}, pretrained: {pretrained}) but not loaded.')

    if output_dict and hasattr(model, "output_dict"):
        model.output_dict = True
    overrides = dict(force_preprocess_cfg or {})
    if getattr(model.visual, 'image_size', None) is not None:
        overrides['size'] = model.visual.image_size         # the size the model was built with wins
    set_model_preprocess_cfg(model, merge_preprocess_dict(asdict(PreprocessCfg()), overrides))
    return model


def _canonical_name(model_name: str) -> str:
    return model_name.replace('/', '-')          # 'ViT-B/32' and 'ViT-B-32' name the same config


def _resolve_architecture(model_name, pretrained, force_quick_gelu, force_patch_dropout, force_image_size, model_kwargs) -> dict:
    if model_name.startswith(HF_HUB_PREFIX):
        raise RuntimeError("hf-hub: models need network access (outside the MI355X hot path)")
    if pretrained and pretrained.lower() == 'openai':
        raise RuntimeError("OpenAI pretrained weights need network access (outside the MI355X hot path)")
    name = _canonical_name(model_name)
    arch = get_model_config(name)
    if arch is None:
        logging.error(f'Model config for {name} not found; available: {list_models()}')
        raise RuntimeError(f'Model config for {name} not found.')
    logging.info(f'Loaded {name} model config.')
    if force_quick_gelu:
        arch["quick_gelu"] = True
    if force_patch_dropout is not None:
        arch["vision_cfg"]["patch_dropout"] = force_patch_dropout
    if force_image_size is not None:
        arch["vision_cfg"]["image_size"] = force_image_size
    arch.update(model_kwargs)                    # explicit keyword arguments override the file
    return arch


def _refuse_unbuilt(arch: dict, jit: bool, pretrained_image: bool, force_custom_text: bool):
    if pretrained_image:
        assert False, 'pretrained image towers currently only supported for timm models'
    if 'timm_model_name' in arch.get('vision_cfg', {}) or 'hf_model_name' in arch.get('text_cfg', {}):
        raise NotImplementedError("timm / HF towers are outside the MI355X hot path")
    if arch.get('custom_text', False) or force_custom_text:
        raise NotImplementedError("CustomTextCLIP is outside the MI355X hot path")
    if jit:
        raise NotImplementedError("torchscript is not supported: the towers are HIP kernel sequences")


def create_model_and_transforms(
        model_name: str,
        pretrained: Optional[str] = None,
        precision: str = 'fp32',
        device: Union[str, torch.device] = 'cpu',
        jit: bool = False,
        force_quick_gelu: bool = False,
        force_custom_text: bool = False,
        force_patch_dropout: Optional[float] = None,
        force_image_size: Optional[Union[int, Tuple[int, int]]] = None,
        image_mean: Optional[Tuple[float, ...]] = None,
        image_std: Optional[Tuple[float, ...]] = None,
        image_interpolation: Optional[str] = None,
        image_resize_mode: Optional[str] = None,  # only effective for inference
        aug_cfg: Optional[Dict[str, Any]] = None,
        pretrained_image: bool = False,
        pretrained_hf: bool = True,
        cache_dir: Optional[str] = None,
        output_dict: Optional[bool] = None,
        **model_kwargs,
):
    force_preprocess_cfg = merge_preprocess_kwargs(
        {}, mean=image_mean, std=image_std, interpolation=image_interpolation, resize_mode=image_resize_mode)
    model = create_model(
        model_name,
        pretrained,
        precision=precision,
        device=device,
        jit=jit,
        force_quick_gelu=force_quick_gelu,
        force_custom_text=force_custom_text,
        force_patch_dropout=force_patch_dropout,
        force_image_size=force_image_size,
        force_preprocess_cfg=force_preprocess_cfg,
        pretrained_image=pretrained_image,
        pretrained_hf=pretrained_hf,
        cache_dir=cache_dir,
        output_dict=output_dict,
        **model_kwargs,
    )
    pp_cfg = PreprocessCfg(**model.visual.preprocess_cfg)
    preprocess_train = TensorImageTransform(pp_cfg, is_train=True)
    preprocess_val = TensorImageTransform(pp_cfg, is_train=False)
    return model, preprocess_train, preprocess_val


def distill_enabled(args) -> bool:
    """Distillation is on when both --distill-model and --distill-pretrained are given (open_clip's trainer)."""
    return bool(getattr(args, "distill_model", None)) and bool(getattr(args, "distill_pretrained", None))


def create_loss(args):
    """Loss module for `args.model` (boundary: reference factory.py:424-461): SigLipLoss under --siglip, DistillClipLoss when
    a teacher is given (--distill-model + --distill-pretrained), ColClipLoss for a colxlip model (global + token-level MaxSim
    contrastive terms mixed by --alpha), ClipLoss otherwise."""
    family = args.model.lower()
    if "coca" in family:
        raise NotImplementedError("CoCaLoss is outside the MI355X hot path")
    if getattr(args, "siglip", False):
        # open_clip's trainer path (the reference's own create_loss reads a --loss-dist-impl its parser never defines)
        assert not getattr(args, "horovod", False), "Horovod not currently supported for SigLip"
        if "colxlip" in family:
            raise ValueError("--siglip needs a CLIP model: a ColXLIP model's output carries token features SigLipLoss cannot take")
        return SigLipLoss(rank=args.rank, world_size=args.world_size, dist_impl=getattr(args, "loss_dist_impl", None))
    common = dict(local_loss=args.local_loss, gather_with_grad=args.gather_with_grad, cache_labels=True,
                  rank=args.rank, world_size=args.world_size, use_horovod=getattr(args, "horovod", False))
    if distill_enabled(args):
        # open_clip's trainer path (the reference parses --distill-model but its main.py:214 never builds a teacher)
        if "colxlip" in family:
            raise ValueError("distillation needs a CLIP student: a ColXLIP model's loss has token-level terms DistillClipLoss "
                             "cannot take")
        return DistillClipLoss(**common)
    if "colxlip" in family:
        return ColClipLoss(alpha=getattr(args, "alpha", 0.5), rows_local=bool(getattr(args, "colclip_rows_local", False)), **common)
    return ClipLoss(**common)
