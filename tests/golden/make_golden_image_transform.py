"""Generate tests/golden/image_transform.npz: uint8 input images and what PIL itself makes of them.

The device image transform (csrc/image_transform.hip) promises PIL's resample -- the one torchvision's RandomResizedCrop /
Resize run on PIL images in the reference's pipeline (open_clip's image_transform_v2, reference factory.py:411-418).  The
fixture therefore stores PIL's own output, `Image.fromarray(img).crop(box).resize((vw, vh), BICUBIC | BILINEAR)` cut to the
output window, for two kinds of image (uniform noise; smooth = an 8x bicubic upsample of noise, rounded) and both filters.
Needs Pillow; the tests only read the .npz.

    python tests/golden/make_golden_image_transform.py

Cases (image h x w, box (top, left, bh, bw), virtual output vh x vw, output window H x W at (oy, ox)); "val" means the
resize-shortest-side + centre-crop geometry of factory.TensorImageTransform for a 32 x 32 output:
    120x160 whole -> 16x16      7.5x / 10x downscale: up to 41 taps
    40x40   whole -> 96x96      upscale
    37x53   (2,1,30,45) -> 16x24   odd sizes, a different scale per axis
    64x48   (14,8,50,40) -> 32x32  crop touching the bottom and right borders
    32x32   whole -> 32x32      identity
    50x70, 70x50, 33x200  val   a window cut from a virtual resized image
and two that reach the kernel's inner loops over a wide or tall source (noise only):
    24x640  whole -> 12x40      16x horizontally: 65 taps, so the output columns are processed in more than one chunk
    256x52  whole -> 16x52      16x vertically: one band of output rows needs more source rows than fit on chip at once
"""
import os

import numpy as np
import torch
import torch.nn.functional as F
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
VAL = 32


def val_geometry(h, w, size=VAL):
    """factory.TensorImageTransform.__call__: scale the shortest side to `size`, centre crop"""
    s = max(size / h, size / w)
    nh, nw = max(size, round(h * s)), max(size, round(w * s))
    return (nh, nw), (size, size), ((nh - size) // 2, (nw - size) // 2)


def cases():
    out = [((120, 160), None, (16, 16), (16, 16), (0, 0)),
           ((40, 40), None, (96, 96), (96, 96), (0, 0)),
           ((37, 53), (2, 1, 30, 45), (16, 24), (16, 24), (0, 0)),
           ((64, 48), (14, 8, 50, 40), (32, 32), (32, 32), (0, 0)),
           ((32, 32), None, (32, 32), (32, 32), (0, 0))]
    for hw in ((50, 70), (70, 50), (33, 200)):
        vsize, win, origin = val_geometry(*hw)
        out.append((hw, None, vsize, win, origin))
    out.append(((24, 640), None, (12, 40), (12, 40), (0, 0)))
    out.append(((256, 52), None, (16, 52), (16, 52), (0, 0)))
    return [(hw, box or (0, 0, hw[0], hw[1]), vsize, win, origin) for hw, box, vsize, win, origin in out]


N_BOTH_KINDS = 8          # the first eight cases come as noise and smooth, the rest as noise only


def make_image(kind, h, w, g):
    if kind == "noise":
        return torch.randint(0, 256, (h, w, 3), generator=g, dtype=torch.uint8).numpy()
    small = torch.randint(0, 256, (1, 3, (h + 7) // 8 + 1, (w + 7) // 8 + 1), generator=g).float()
    up = F.interpolate(small, scale_factor=8, mode="bicubic", align_corners=False)[0, :, :h, :w]
    return up.round().clamp(0, 255).to(torch.uint8).permute(1, 2, 0).contiguous().numpy()


def main():
    g = torch.Generator().manual_seed(20240607)
    arrays = {}
    geom = []
    for ci, (hw, box, vsize, win, origin) in enumerate(cases()):
        geom.append([*hw, *box, *vsize, *win, *origin])
        top, left, bh, bw = box
        for kind in (("noise", "smooth") if ci < N_BOTH_KINDS else ("noise",)):
            img = make_image(kind, hw[0], hw[1], g)
            arrays[f"img_{kind}_{ci}"] = img
            for name, flt in (("bicubic", Image.BICUBIC), ("bilinear", Image.BILINEAR)):
                res = Image.fromarray(img).crop((left, top, left + bw, top + bh)).resize((vsize[1], vsize[0]), flt)
                res = np.asarray(res)[origin[0]:origin[0] + win[0], origin[1]:origin[1] + win[1]]
                arrays[f"pil_{kind}_{name}_{ci}"] = np.ascontiguousarray(res)
    arrays["geometry"] = np.asarray(geom, dtype=np.int64)      # h, w, top, left, bh, bw, vh, vw, H, W, oy, ox
    path = os.path.join(HERE, "image_transform.npz")
    np.savez_compressed(path, **arrays)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
