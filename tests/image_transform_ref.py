"""Test helper: the two-pass resample that csrc/image_transform.hip implements, restated in numpy (coefficients in 22-bit fixed
point, integer sums, as PIL's Resample.c does for 8-bit channels), and the three bounds a result must meet against PIL's own
output.  It lives with the tests because the product has no CPU path."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "image_transform.npz")
N_BOTH_KINDS = 8          # golden cases 0..7 exist as noise and smooth images, the later ones as noise only

# against PIL: every pixel within 1 level; differing pixels at most 1 % (bicubic) / 8 % (bilinear) per case; |mean signed
# difference| at most 0.06 level.  The margin is what an fp32 sum needs, because it breaks exact .5 ties differently from PIL's
# fixed point; the fixed-point restatement below (and the kernel) is expected to differ nowhere.
MAX_LEVEL_DIFF = 1
MAX_DIFF_FRACTION = {"bicubic": 0.01, "bilinear": 0.08}
MAX_BIAS = 0.06
PRECISION_BITS = 22       # PIL: 32 - 8 - 2


def load_cases():
    """[(case number, kind, uint8 image [h,w,3], geometry dict, {'bicubic': PIL output, 'bilinear': PIL output})]"""
    z = np.load(GOLDEN)
    keys = ("h", "w", "top", "left", "bh", "bw", "vh", "vw", "H", "W", "oy", "ox")
    out = []
    for ci, row in enumerate(z["geometry"]):
        geo = dict(zip(keys, (int(v) for v in row)))
        for kind in (("noise", "smooth") if ci < N_BOTH_KINDS else ("noise",)):
            out.append((ci, kind, z[f"img_{kind}_{ci}"], geo,
                        {name: z[f"pil_{kind}_{name}_{ci}"] for name in ("bicubic", "bilinear")}))
    return out


def _filter(name, x):
    x = np.abs(x)
    if name == "bilinear":
        return np.where(x < 1.0, 1.0 - x, 0.0)
    a = -0.5
    return np.where(x < 1.0, ((a + 2.0) * x - (a + 3.0)) * x * x + 1.0,
                    np.where(x < 2.0, (((x - 5.0) * x + 8.0) * x - 4.0) * a, 0.0))


def coefficients(name, n_in, n_out, i):
    """(lo, 22-bit fixed-point weights) of output index i of an axis resampled from n_in to n_out pixels"""
    scale = n_in / n_out
    fs = max(scale, 1.0)
    support = (2.0 if name == "bicubic" else 1.0) * fs
    center = (i + 0.5) * scale
    lo = max(0, int(center - support + 0.5))
    hi = min(n_in, int(center + support + 0.5))
    w = _filter(name, (np.arange(lo, hi) - center + 0.5) * (1.0 / fs))
    total = 0.0
    for v in w:                                       # summed in order, as PIL does
        total += float(v)
    k = w / total * float(1 << PRECISION_BITS)
    return lo, np.where(k < 0, -0.5 + k, 0.5 + k).astype(np.int64)                 # (int) truncates toward zero


def _pass(name, src, n_out, first, count):
    """resample axis 0 of integer src [n_in, ...] to outputs first .. first+count of a virtual n_out; rounded half up, clamped"""
    out = np.empty((count,) + src.shape[1:], dtype=np.int64)
    for k in range(count):
        lo, w = coefficients(name, src.shape[0], n_out, first + k)
        acc = np.full(src.shape[1:], 1 << (PRECISION_BITS - 1), dtype=np.int64)
        for t in range(len(w)):
            acc = acc + src[lo + t] * w[t]
        out[k] = np.clip(acc >> PRECISION_BITS, 0, 255)
    return out


def resample_levels(img, geo, name):
    """uint8 levels [H, W, 3] of the window of geo: horizontal pass over the boxed region, round, vertical pass, round"""
    box = img[geo["top"]:geo["top"] + geo["bh"], geo["left"]:geo["left"] + geo["bw"]].astype(np.int64)
    horiz = _pass(name, box.transpose(1, 0, 2), geo["vw"], geo["ox"], geo["W"]).transpose(1, 0, 2)     # [bh, W, 3]
    return _pass(name, horiz, geo["vh"], geo["oy"], geo["H"]).astype(np.uint8)


def compare_with_pil(levels, pil, name):
    """(max |difference|, fraction of differing pixels, |mean signed difference|) in levels"""
    d = levels.astype(np.int64) - pil.astype(np.int64)
    return int(np.abs(d).max()), float((d != 0).mean()), abs(float(d.mean()))


def assert_within_pil_bounds(levels, pil, name, what=""):
    worst, frac, bias = compare_with_pil(levels, pil, name)
    print(f"{what} {name}: max diff {worst}, differing {100 * frac:.2f} %, bias {bias:.4f}")
    assert levels.shape == pil.shape, (what, levels.shape, pil.shape)
    assert worst <= MAX_LEVEL_DIFF, (what, name, worst)
    assert frac <= MAX_DIFF_FRACTION[name], (what, name, frac)
    assert bias <= MAX_BIAS, (what, name, bias)
