"""The device image transform on the GPU: `ops.image_transform` against PIL's own outputs (tests/golden/image_transform.npz) in one
ragged launch, normalisation and bf16 output, the scale limit, the packed loader's buffer reuse, and `main` training and
evaluating on a packed directory."""
import json
import logging
import math
import os
import re

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from colxlip_amd import ops  # noqa: E402
from colxlip_amd.data import PackedDataset, PackedLoader  # noqa: E402
from colxlip_amd.factory import OPENAI_DATASET_MEAN, OPENAI_DATASET_STD, HashTokenizer, PreprocessCfg  # noqa: E402
from colxlip_amd.image_transform import DeviceImageTransform  # noqa: E402
from colxlip_amd.main import main  # noqa: E402
from colxlip_amd.pack import write_packed  # noqa: E402
from tests import image_transform_ref as R  # noqa: E402

DEV = "cuda:0"
OUT = (96, 96)            # the largest window of the golden cases; smaller ones leave the rest of their 96 x 96 untouched
SENTINEL = -7.0


class _Ragged:
    """every golden (case, kind) image in ONE byte buffer: shuffled order, a leading pad, 64-byte alignment with gaps"""

    def __init__(self):
        self.cases = R.load_cases()
        order = np.random.default_rng(0).permutation(len(self.cases))
        offsets, pos, chunks = np.zeros(len(self.cases), dtype=np.int64), 192, [np.zeros(192, dtype=np.uint8)]
        for i in order:
            img = self.cases[i][2]
            offsets[i] = pos
            pad = (-img.size) % 64 + 64 * int(i % 2)
            chunks += [img.reshape(-1), np.full(pad, 255, dtype=np.uint8)]
            pos += img.size + pad
        self.data = torch.from_numpy(np.concatenate(chunks)).to(DEV)
        geo = [c[3] for c in self.cases]
        self.meta = ops.image_geometry(offsets, [[g["h"], g["w"]] for g in geo], [[g["top"], g["left"], g["bh"], g["bw"]] for g in geo],
                                       [[g["vh"], g["vw"]] for g in geo], [[g["oy"], g["ox"]] for g in geo], OUT,
                                       self.data.numel(), allow_partial=True).to(DEV)
        self._levels = {}

    def run(self, name, mean=(0.0, 0.0, 0.0), std=(1.0, 1.0, 1.0), dtype=torch.float32):
        out = torch.full((len(self.cases), 3) + OUT, SENTINEL, dtype=dtype, device=DEV)
        ops.image_transform(self.data, self.meta, OUT, mean, std, name, dtype, out=out)
        torch.cuda.synchronize()
        return out.cpu()

    def levels(self, name):
        """255 * out of the mean 0 / std 1 fp32 run: float [n, 3, 96, 96], computed once per filter"""
        if name not in self._levels:
            self._levels[name] = 255.0 * self.run(name)
        return self._levels[name]

    def window(self, i):
        g = self.cases[i][3]
        return slice(0, g["H"]), slice(0, g["W"])

    def written(self, i):
        """what the kernel may write of the 96 x 96 output: the window, clipped to the virtual output (for a val case the virtual
        image goes on to the right of / below its 32 x 32 window)"""
        g = self.cases[i][3]
        return slice(0, min(OUT[0], g["vh"] - g["oy"])), slice(0, min(OUT[1], g["vw"] - g["ox"]))


@pytest.fixture(scope="module")
def ragged():
    return _Ragged()


# ---------------------------------------------------------------------------------------------------------- kernel vs PIL
@pytest.mark.parametrize("name", ["bicubic", "bilinear"])
def test_kernel_matches_pil_in_one_ragged_launch(ragged, name):
    """All golden cases (mixed sizes, crops, up- and downscales to 65 taps, val windows, chunked columns, split row groups) in one
    launch.  255 * out is an integer level to 1e-3; the levels are within 1 of PIL's everywhere, differ in at most 1 % (bicubic) /
    8 % (bilinear) of a case's pixels, and are unbiased to 0.06 level; what lies beyond a case's virtual output is not written."""
    lv = ragged.levels(name)
    for i, (ci, kind, img, geo, pil) in enumerate(ragged.cases):
        ys, xs = ragged.window(i)
        got = lv[i, :, ys, xs]
        assert float((got - got.round()).abs().max()) <= 1e-3, (ci, kind)
        levels = got.round().permute(1, 2, 0).numpy().astype(np.int64)
        assert levels.min() >= 0 and levels.max() <= 255
        R.assert_within_pil_bounds(levels, pil[name], name, f"case {ci} {kind}")
        untouched = lv[i].clone()
        wy, wx = ragged.written(i)
        untouched[:, wy, wx] = 255.0 * SENTINEL
        assert bool((untouched == 255.0 * SENTINEL).all()), (ci, kind)


def test_normalisation_and_bf16(ragged):
    """With the OpenAI mean / std, fp32 output = (level / 255 - mean) / std of the first run's levels to 1e-6, and bf16 output is
    that value rounded to bf16."""
    lv = ragged.levels("bicubic").round()
    mean = torch.tensor(OPENAI_DATASET_MEAN, dtype=torch.float32).view(1, 3, 1, 1)
    std = torch.tensor(OPENAI_DATASET_STD, dtype=torch.float32).view(1, 3, 1, 1)
    want = (lv / 255.0 - mean) / std
    f32 = ragged.run("bicubic", OPENAI_DATASET_MEAN, OPENAI_DATASET_STD, torch.float32)
    b16 = ragged.run("bicubic", OPENAI_DATASET_MEAN, OPENAI_DATASET_STD, torch.bfloat16)
    assert b16.dtype == torch.bfloat16
    for i in range(len(ragged.cases)):
        ys, xs = ragged.window(i)
        err = float((f32[i, :, ys, xs] - want[i, :, ys, xs]).abs().max())
        print(f"case {ragged.cases[i][0]} {ragged.cases[i][1]}: fp32 max error {err:.3e}")
        assert err <= 1e-6
        assert torch.equal(b16[i, :, ys, xs], want[i, :, ys, xs].to(torch.bfloat16))
        rest = b16[i].float().clone()
        wy, wx = ragged.written(i)
        rest[:, wy, wx] = SENTINEL
        assert bool((rest == SENTINEL).all())


# ------------------------------------------------------------------------------------------------------------ scale limit
def _pack(root, sizes, seed=0, K=1):
    rng = np.random.default_rng(seed)
    images = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in sizes]
    captions = [[f"caption {k} of image {i} word{i % 5}" for k in range(K)] for i in range(len(sizes))]
    write_packed(str(root), images, captions, HashTokenizer(77, 512), tokenizer_name="hash")
    return images


def test_scale_above_16_raises_before_any_launch(tmp_path, monkeypatch):
    launches = []
    real = ops.image_transform
    monkeypatch.setattr(ops, "image_transform", lambda *a, **k: (launches.append(1), real(*a, **k))[1])
    t = DeviceImageTransform(PreprocessCfg(size=32), is_train=True)
    with pytest.raises(ValueError, match="16x"):
        t.geometry([0], [[600, 40]], 3 * 600 * 40, boxes=[[0, 0, 600, 40]])
    assert t.geometry([0], [[512, 40]], 3 * 512 * 40, boxes=[[0, 0, 512, 40]]).shape == (1, 6)         # exactly 16x passes
    _pack(tmp_path / "big", [(800, 800)] * 2)          # every crop of >= 90 % of the area is > 16 x 32 tall
    loader = PackedLoader(str(tmp_path / "big"), 2, t, DEV)
    with pytest.raises(ValueError, match="16x"):
        next(iter(loader))
    assert launches == []


# ------------------------------------------------------------------------------------------------------------------ loader
def _reference_batch(ds, transform, idx, generator, dtype):
    """the transform of images idx with the boxes drawn from `generator`, through a buffer of its own"""
    imgs = [np.ascontiguousarray(ds.image(int(i))) for i in idx]
    offsets = np.cumsum([0] + [im.size for im in imgs[:-1]])
    data = torch.from_numpy(np.concatenate([im.reshape(-1) for im in imgs])).to(DEV)
    hw = [[im.shape[0], im.shape[1]] for im in imgs]
    meta = transform.geometry(offsets, hw, data.numel(), generator)
    return transform(data, meta, dtype)


def test_loader_batches_survive_buffer_reuse(tmp_path):
    """Batch k is taken, then batches k+1 and k+2 (k+2 refills k's staging and device buffers): batch k must still be the
    transform of its images with its boxes.  Checked for every batch of two epochs, tokens included."""
    rng = np.random.default_rng(1)
    sizes = [(int(rng.integers(40, 71)), int(rng.integers(40, 71))) for _ in range(14)]
    _pack(tmp_path / "ds", sizes, K=2)
    ds = PackedDataset(str(tmp_path / "ds"))
    t = DeviceImageTransform(PreprocessCfg(size=32), is_train=True, aug_cfg={"scale": (0.3, 1.0)})
    loader = PackedLoader(ds, 2, t, DEV, seed=9, workers=3)
    assert loader.num_batches == 7
    for epoch in (0, 1):
        loader.set_epoch(epoch)
        it = iter(loader)
        held = [next(it) for _ in range(3)]                   # k, k+1, k+2 in flight at once
        held += list(it)
        torch.cuda.synchronize()
        plan = loader.plan(epoch)
        assert len(held) == len(plan) == 7
        for k, ((idx, _), (images, texts)) in enumerate(zip(plan, held)):
            assert images.shape == (2, 3, 32, 32) and images.dtype == torch.float32 and images.is_cuda
            assert texts.shape == (2, 2, 77) and texts.dtype == torch.int64 and texts.is_cuda
            want = _reference_batch(ds, t, idx, loader.batch_generator(epoch, k), torch.float32)
            assert torch.equal(images, want), (epoch, k)
            assert np.array_equal(texts.cpu().numpy(), ds.tokens[idx].astype(np.int64)), (epoch, k)
    first = [b[0].clone() for b in held[:2]]
    loader.set_epoch(1)
    again = [b[0] for _, b in zip(range(2), loader)]          # an iteration abandoned half way, then the same epoch again
    assert all(torch.equal(a, b) for a, b in zip(first, again))


# -------------------------------------------------------------------------------------------------------------- end to end
def _train(tmp_path, name, data_dir, caplog, extra=()):
    argv = ["--model", "ViT-tiny-test", "--dataset-type", "packed", "--train-data", data_dir, "--precision", "fp32",
            "--batch-size", "8", "--epochs", "2", "--lr", "1e-3", "--warmup", "1", "--workers", "2", "--seed", "3",
            "--logs-dir", str(tmp_path), "--name", name, "--log-every-n-steps", "1", *extra]
    with caplog.at_level(logging.INFO):
        caplog.clear()
        assert main(argv) == 0
    lines = [r.getMessage() for r in caplog.records if r.getMessage().startswith("Train Epoch")]
    return [float(re.search(r"Total_loss: ([\d.eE+-]+|nan|inf)", l).group(1)) for l in lines]


def test_main_trains_and_evaluates_on_a_packed_directory(tmp_path, caplog):
    rng = np.random.default_rng(2)
    sizes = [(int(rng.integers(40, 71)), int(rng.integers(40, 71))) for _ in range(24)]
    _pack(tmp_path / "train", sizes, K=2)
    _pack(tmp_path / "val", sizes[:10], seed=5, K=2)
    a = _train(tmp_path, "a", str(tmp_path / "train"), caplog)
    b = _train(tmp_path, "b", str(tmp_path / "train"), caplog)
    assert len(a) == 6 and all(math.isfinite(v) for v in a), a            # 2 epochs x 3 batches of 8
    assert a == b, (a, b)
    _train(tmp_path, "c", str(tmp_path / "train"), caplog, ["--retrieval-coco", "--val-data", str(tmp_path / "val")])
    with open(os.path.join(tmp_path, "c", "checkpoints", "results.jsonl")) as f:
        rows = [json.loads(l) for l in f]
    assert len(rows) == 2                                                   # after each epoch
    keys = [k for k in rows[-1] if k.startswith("retrieval_coco")]
    assert any("num_image_samples" in k for k in keys) and any("R@1" in k or "r@1" in k.lower() for k in keys), rows[-1]
    assert [v for k, v in rows[-1].items() if "num_image_samples" in k] == [10]
    assert [v for k, v in rows[-1].items() if "num_text_samples" in k] == [20]
