"""Geometry of the device image transform: where the reference's train / val pipelines (open_clip's image_transform_v2,
reference factory.py:411-418) look in each image.  The pixels are `ops.image_transform` (csrc/image_transform.hip); this
module only decides, on the host, the source box, the virtual output size and the output window of every image.

  train  RandomResizedCrop(size, scale, ratio) : box = the random crop, virtual output = size, window origin 0
  val    Resize(shortest side) + CenterCrop    : box = the image, virtual output = the resized image, window = the centre crop
         (emitting only the window equals resizing and then cropping: the two resample passes are separable)
"""
import math
from typing import Optional, Sequence, Tuple

import torch

from . import ops

# open_clip.transform.AugmentationCfg defaults
DEFAULT_SCALE = (0.9, 1.0)
DEFAULT_RATIO = (3.0 / 4.0, 4.0 / 3.0)
_ATTEMPTS = 10


def parse_aug_cfg(aug_cfg) -> Tuple[Tuple[float, float], Tuple[float, float]]:
    """(scale, ratio) from `--aug-cfg scale=(lo,hi) ratio=(lo,hi)`.  The other AugmentationCfg keys (color jitter, re-prob, timm
    augmentation, ...) have no device implementation here and are refused rather than ignored."""
    cfg = dict(aug_cfg or {})
    unknown = sorted(set(cfg) - {"scale", "ratio"})
    if unknown:
        raise ValueError(f"--aug-cfg: {', '.join(unknown)} not supported by the device image transform (supported: scale, ratio)")
    out = []
    for key, default in (("scale", DEFAULT_SCALE), ("ratio", DEFAULT_RATIO)):
        val = cfg.get(key, default)
        if not (isinstance(val, (tuple, list)) and len(val) == 2 and 0 < float(val[0]) <= float(val[1])):
            raise ValueError(f"--aug-cfg {key}={val!r}: expected (low, high) with 0 < low <= high")
        out.append((float(val[0]), float(val[1])))
    return out[0], out[1]


def random_resized_crop_boxes(hw, scale=DEFAULT_SCALE, ratio=DEFAULT_RATIO, generator: Optional[torch.Generator] = None,
                              return_accepted: bool = False):
    """Crop boxes (top, left, bh, bw), int64 [n, 4], for images of sizes hw [n, 2]: torchvision's
    `transforms.RandomResizedCrop.get_params` (torchvision/transforms/transforms.py), restated for a whole batch at once.
    Up to 10 attempts per image: target area = h*w * U(scale), aspect = exp(U(log ratio)), bw = round(sqrt(area * aspect)),
    bh = round(sqrt(area / aspect)); the first attempt that fits is placed at a uniform integer (top, left).  An image none
    fits gets the centred fallback: the whole image clamped to the ratio bounds."""
    hw = torch.as_tensor(hw, dtype=torch.int64).reshape(-1, 2)
    n = hw.shape[0]
    h, w = hw[:, 0], hw[:, 1]
    u = torch.rand((n, 2 * _ATTEMPTS + 2), generator=generator, dtype=torch.float64)
    area = (h * w).to(torch.float64)[:, None] * (scale[0] + (scale[1] - scale[0]) * u[:, :_ATTEMPTS])
    log_lo, log_hi = math.log(ratio[0]), math.log(ratio[1])
    aspect = torch.exp(log_lo + (log_hi - log_lo) * u[:, _ATTEMPTS:2 * _ATTEMPTS])
    bw = torch.round(torch.sqrt(area * aspect)).to(torch.int64)
    bh = torch.round(torch.sqrt(area / aspect)).to(torch.int64)
    fits = (bw > 0) & (bw <= w[:, None]) & (bh > 0) & (bh <= h[:, None])
    accepted = fits.any(dim=1)
    first = fits.to(torch.int64).argmax(dim=1)[:, None]               # first fitting attempt (0 when none: replaced below)
    bw, bh = bw.gather(1, first)[:, 0], bh.gather(1, first)[:, 0]
    top = torch.floor(u[:, -2] * (h - bh + 1).to(torch.float64)).to(torch.int64)
    left = torch.floor(u[:, -1] * (w - bw + 1).to(torch.float64)).to(torch.int64)
    # fallback: central crop of the whole image, its aspect clamped to the ratio bounds
    in_ratio = w.to(torch.float64) / h.to(torch.float64)
    fw, fh = w.clone(), h.clone()
    narrow, wide = in_ratio < min(ratio), in_ratio > max(ratio)
    fh = torch.where(narrow, torch.round(w.to(torch.float64) / min(ratio)).to(torch.int64), fh)
    fw = torch.where(wide, torch.round(h.to(torch.float64) * max(ratio)).to(torch.int64), fw)
    fh, fw = torch.minimum(fh, h).clamp(min=1), torch.minimum(fw, w).clamp(min=1)
    box = torch.stack([torch.where(accepted, top, (h - fh) // 2), torch.where(accepted, left, (w - fw) // 2),
                       torch.where(accepted, bh, fh), torch.where(accepted, bw, fw)], dim=1)
    return (box, accepted) if return_accepted else box


def center_crop_geometry(hw, size) -> Tuple[torch.Tensor, torch.Tensor]:
    """(virtual output (vh, vw) [n, 2], window origin (oy, ox) [n, 2]) of resize-shortest-side + centre crop to `size`: the
    arithmetic of `factory.TensorImageTransform.__call__` (scale = max(H / h, W / w), each side rounded, never below the crop)."""
    hw = torch.as_tensor(hw, dtype=torch.int64).reshape(-1, 2)
    H, W = size
    rows = []
    for h, w in hw.tolist():
        s = max(H / h, W / w)
        nh, nw = max(H, round(h * s)), max(W, round(w * s))
        rows.append((nh, nw, (nh - H) // 2, (nw - W) // 2))
    g = torch.tensor(rows, dtype=torch.int64).reshape(-1, 4)
    return g[:, :2].contiguous(), g[:, 2:].contiguous()


class DeviceImageTransform:
    """Train or val image pipeline on the device for one preprocess configuration (`factory.PreprocessCfg`).
    `geometry(...)` decides, on the host, where to look in each image and returns the kernel's validated records;
    `__call__(data, meta)` runs the kernel on a device byte buffer."""

    def __init__(self, cfg, is_train: bool, aug_cfg=None):
        size = cfg.size if isinstance(cfg.size, (tuple, list)) else (cfg.size, cfg.size)
        self.size = (int(size[0]), int(size[1]))
        self.mean, self.std = tuple(cfg.mean), tuple(cfg.std)
        if cfg.interpolation not in ("bicubic", "bilinear"):
            raise ValueError(f"device image transform: interpolation {cfg.interpolation!r} is not built (bicubic | bilinear)")
        if not is_train and getattr(cfg, "resize_mode", "shortest") != "shortest":
            raise ValueError(f"device image transform: resize mode {cfg.resize_mode!r} is not built (shortest)")
        self.interpolation = cfg.interpolation
        self.is_train = is_train
        self.scale, self.ratio = parse_aug_cfg(aug_cfg)

    def boxes(self, hw, generator: Optional[torch.Generator] = None) -> torch.Tensor:
        """source boxes [n, 4]: random resized crops when training, whole images otherwise"""
        hw = torch.as_tensor(hw, dtype=torch.int64).reshape(-1, 2)
        if self.is_train:
            return random_resized_crop_boxes(hw, self.scale, self.ratio, generator)
        return torch.cat([torch.zeros_like(hw), hw], dim=1)

    def geometry(self, offsets, hw, nbytes: int, generator: Optional[torch.Generator] = None, boxes=None) -> torch.Tensor:
        """kernel records (`ops.image_geometry`) for images of sizes hw at `offsets` of a buffer of `nbytes`"""
        hw = torch.as_tensor(hw, dtype=torch.int64).reshape(-1, 2)
        n = hw.shape[0]
        if boxes is None:
            boxes = self.boxes(hw, generator)
        if self.is_train:
            vsize = torch.tensor(self.size, dtype=torch.int64).repeat(n, 1)
            origin = torch.zeros((n, 2), dtype=torch.int64)
        else:
            vsize, origin = center_crop_geometry(hw, self.size)
        return ops.image_geometry(offsets, hw, boxes, vsize, origin, self.size, nbytes)

    def __call__(self, data: torch.Tensor, meta: torch.Tensor, dtype=torch.float32) -> torch.Tensor:
        return ops.image_transform(data, meta, self.size, self.mean, self.std, self.interpolation, dtype)

    def __repr__(self):
        return (f"DeviceImageTransform(size={self.size}, train={self.is_train}, interpolation={self.interpolation}"
                + (f", scale={self.scale}, ratio={self.ratio})" if self.is_train else ")"))


def transform_from(preprocess_fn, is_train: bool, aug_cfg=None, size: Optional[Sequence[int]] = None) -> DeviceImageTransform:
    """The device pipeline for what `create_model_and_transforms` returned (its transforms carry the PreprocessCfg as `.cfg`)."""
    from .factory import PreprocessCfg
    cfg = getattr(preprocess_fn, "cfg", None) or PreprocessCfg()
    if size is not None:
        from dataclasses import replace
        cfg = replace(cfg, size=tuple(size) if isinstance(size, (tuple, list)) else size)
    return DeviceImageTransform(cfg, is_train, aug_cfg)
