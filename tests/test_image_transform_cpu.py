"""Host side of the real-image input path: the resample semantics the kernel is written to (restated in numpy, against PIL's own
output), crop-box drawing, the packed dataset's writer and reader, and the loader's epoch / rank partition.  No GPU needed."""
import os

import numpy as np
import pytest
import torch

from colxlip_amd import create_model_and_transforms, ops
from colxlip_amd.data import PackedDataset, PackedLoader, get_data
from colxlip_amd.factory import HashTokenizer, PreprocessCfg
from colxlip_amd.image_transform import (DeviceImageTransform, center_crop_geometry, parse_aug_cfg,
                                         random_resized_crop_boxes)
from colxlip_amd.pack import main as pack_main, write_packed
from colxlip_amd.params import parse_args
from tests import image_transform_ref as R

CASES = R.load_cases()


# ---------------------------------------------------------------------------------------------------------- resample semantics
@pytest.mark.parametrize("name", ["bicubic", "bilinear"])
def test_restated_resample_matches_pil(name):
    """The two-pass resample as the kernel implements it (fixed-point sums, rounded half up and clamped after each pass) stays within
    1 level of PIL everywhere, differs in at most 1 % (bicubic) / 8 % (bilinear) of the pixels of a case, and is unbiased to 0.06
    level -- on every golden case, noise and smooth."""
    assert len(CASES) == 18
    for ci, kind, img, geo, pil in CASES:
        assert img.shape == (geo["h"], geo["w"], 3) and pil[name].shape == (geo["H"], geo["W"], 3)
        R.assert_within_pil_bounds(R.resample_levels(img, geo, name), pil[name], name, f"case {ci} {kind}")


def test_single_float_pass_is_not_pil():
    """Why two rounded passes: one float pass without the intermediate rounding leaves PIL by more than a level on noise."""
    ci, kind, img, geo, pil = CASES[0]
    assert kind == "noise"
    box = img.astype(np.float32)
    cols = [R.coefficients("bicubic", geo["bw"], geo["vw"], x) for x in range(geo["W"])]
    rows = [R.coefficients("bicubic", geo["bh"], geo["vh"], y) for y in range(geo["H"])]
    horiz = np.stack([sum(box[:, lo + t] * w[t] for t in range(len(w))) for lo, w in cols], axis=1)
    full = np.stack([sum(horiz[lo + t] * w[t] for t in range(len(w))) for lo, w in rows], axis=0)
    once = np.clip(np.floor(full + 0.5), 0, 255)
    assert np.abs(once - R.resample_levels(img, geo, "bicubic")).max() >= 1


def test_val_geometry_is_the_tensor_transforms():
    """the val cases of the fixture were cut with factory.TensorImageTransform's resize-shortest + centre-crop arithmetic"""
    for ci in (5, 6, 7):
        geo = [c for c in CASES if c[0] == ci][0][3]
        vsize, origin = center_crop_geometry([[geo["h"], geo["w"]]], (32, 32))
        assert vsize.tolist() == [[geo["vh"], geo["vw"]]] and origin.tolist() == [[geo["oy"], geo["ox"]]]
        assert min(geo["vh"], geo["vw"]) == 32
    t = DeviceImageTransform(PreprocessCfg(size=32), is_train=False)
    meta = t.geometry([0], [[50, 70]], 3 * 50 * 70)
    assert meta.view(torch.int32)[0, 2:].tolist() == [50, 70, 0, 0, 50, 70, 32, 45, 0, 6]


def test_geometry_is_validated_on_the_host():
    ok = dict(offsets=[0], hw=[[40, 60]], box=[[0, 0, 40, 60]], vsize=[[32, 32]], origin=[[0, 0]], out_hw=(32, 32), nbytes=7200)
    meta = ops.image_geometry(**ok)
    assert meta.dtype == torch.int64 and meta.shape == (1, 6) and int(meta[0, 0]) == 0
    for bad in (dict(nbytes=7199), dict(box=[[0, 0, 41, 60]]), dict(box=[[0, 1, 40, 60]]), dict(origin=[[1, 0]]),
                dict(offsets=[-1]), dict(vsize=[[32, 3]]), dict(hw=[[40, 0]])):
        with pytest.raises(ValueError):
            ops.image_geometry(**{**ok, **bad})
    # the scale limit: 16x is accepted, anything above is refused
    ops.image_geometry([0], [[512, 40]], [[0, 0, 512, 40]], [[32, 32]], [[0, 0]], (32, 32), 3 * 512 * 40)
    with pytest.raises(ValueError, match="16x"):
        ops.image_geometry([0], [[513, 40]], [[0, 0, 513, 40]], [[32, 32]], [[0, 0]], (32, 32), 3 * 513 * 40)
    assert ops.image_geometry(**{**ok, "origin": [[1, 0]], "allow_partial": True}).shape == (1, 6)


# ---------------------------------------------------------------------------------------------------------------- crop boxes
def test_random_resized_crop_boxes():
    g = torch.Generator().manual_seed(3)
    hw = torch.stack([torch.randint(40, 400, (500,), generator=g), torch.randint(40, 400, (500,), generator=g)], dim=1)
    scale, ratio = (0.3, 1.0), (3 / 4, 4 / 3)
    box, accepted = random_resized_crop_boxes(hw, scale, ratio, torch.Generator().manual_seed(0), return_accepted=True)
    top, left, bh, bw = box.unbind(1)
    assert box.dtype == torch.int64 and box.shape == (500, 4)
    assert bool(((top >= 0) & (left >= 0) & (bh >= 1) & (bw >= 1) & (top + bh <= hw[:, 0]) & (left + bw <= hw[:, 1])).all())
    assert int(accepted.sum()) > 400
    # accepted boxes: area and aspect inside the ranges, up to the rounding of the two sides to integers
    area = (bh * bw).double() / (hw[:, 0] * hw[:, 1]).double()
    aspect = bw.double() / bh.double()
    slack = 1.0 / bh.double() + 1.0 / bw.double()
    a = accepted
    assert bool((area[a] >= scale[0] * (1 - slack[a])).all()) and bool((area[a] <= scale[1] * (1 + slack[a])).all())
    assert bool((aspect[a] >= ratio[0] * (1 - slack[a])).all()) and bool((aspect[a] <= ratio[1] * (1 + slack[a])).all())
    assert len(set(top[a].tolist())) > 20 and len(set(left[a].tolist())) > 20          # placed, not centred
    # same generator state, same boxes
    again = random_resized_crop_boxes(hw, scale, ratio, torch.Generator().manual_seed(0))
    assert torch.equal(again, box)


def test_crop_fallback_on_an_extreme_aspect():
    """10 x 200: no crop with aspect <= 4/3 and >= 90 % of the area fits, so the centred fallback clamps the aspect"""
    box, accepted = random_resized_crop_boxes([[10, 200], [200, 10]], generator=torch.Generator().manual_seed(1), return_accepted=True)
    assert accepted.tolist() == [False, False]
    assert box.tolist() == [[0, (200 - 13) // 2, 10, 13], [(200 - 13) // 2, 0, 13, 10]]      # round(10 * 4/3) = 13


def test_aug_cfg_keys():
    assert parse_aug_cfg({}) == ((0.9, 1.0), (3 / 4, 4 / 3))
    assert parse_aug_cfg({"scale": (0.5, 1.0), "ratio": (1.0, 1.0)}) == ((0.5, 1.0), (1.0, 1.0))
    args = parse_args(["--model", "ViT-tiny-test", "--aug-cfg", "scale=(0.4,1.0)"])
    assert parse_aug_cfg(args.aug_cfg)[0] == (0.4, 1.0)
    with pytest.raises(ValueError, match="color_jitter"):
        parse_aug_cfg({"color_jitter": 0.4})
    with pytest.raises(ValueError):
        parse_aug_cfg({"scale": 0.5})


# ------------------------------------------------------------------------------------------------------- pack and loader
def _write_pngs(root, n, seed=0):
    from PIL import Image
    rng = np.random.default_rng(seed)
    os.makedirs(root, exist_ok=True)
    rows = ["filepath\ttitle"]
    for i in range(n):
        h, w = int(rng.integers(40, 71)), int(rng.integers(40, 71))
        arr = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        mode = "RGB" if i % 3 else "L"                                   # a grey file: convert('RGB') must apply
        Image.fromarray(arr if mode == "RGB" else arr[:, :, 0], mode).save(os.path.join(root, f"im{i}.png"))
        rows.append(f"im{i}.png\ta photo number {i}|||picture {i} again")
    with open(os.path.join(root, "captions.tsv"), "w") as f:
        f.write("\n".join(rows) + "\n")
    return os.path.join(root, "captions.tsv")


@pytest.fixture(scope="module")
def packed_dir(tmp_path_factory):
    root = tmp_path_factory.mktemp("packed")
    table = _write_pngs(str(root / "src"), 12)
    out = str(root / "ds")
    assert pack_main(["--csv", table, "--model", "ViT-tiny-test", "--out", out]) == 0
    return str(root / "src"), out


def test_pack_round_trip(packed_dir):
    from PIL import Image
    src, out = packed_dir
    ds = PackedDataset(out)
    assert len(ds) == 12 and ds.K == 2 and ds.meta["n"] == 12 and ds.meta["K"] == 2
    assert ds.index.dtype == np.int64 and ds.tokens.dtype == np.int32 and ds.tokens.shape == (12, 2, ds.context_length)
    assert bool((ds.index[:, 0] % 64 == 0).all())
    tok = HashTokenizer(ds.context_length, ds.meta["vocab_size"])
    for i in range(12):
        want = np.asarray(Image.open(os.path.join(src, f"im{i}.png")).convert("RGB"))
        assert np.array_equal(ds.image(i), want)                          # byte-identical to PIL decode
        assert np.array_equal(ds.tokens[i], tok([f"a photo number {i}", f"picture {i} again"]).numpy())
    assert len({tuple(ds.index[i, 1:]) for i in range(12)}) > 6           # mixed sizes
    with pytest.raises(FileNotFoundError):
        PackedDataset(src)


def test_pack_max_side_and_caption_count(tmp_path):
    from colxlip_amd.pack import decode_rgb
    from PIL import Image
    Image.fromarray(np.zeros((90, 300, 3), dtype=np.uint8)).save(tmp_path / "wide.png")
    assert decode_rgb(tmp_path / "wide.png", max_side=30).shape == (30, 100, 3)
    assert decode_rgb(tmp_path / "wide.png", max_side=128).shape == (90, 300, 3)
    with pytest.raises(ValueError, match="same"):
        write_packed(str(tmp_path / "bad"), [np.zeros((4, 4, 3), np.uint8)] * 2, [["a"], ["a", "b"]], HashTokenizer(16, 512))


@pytest.mark.parametrize("world", [1, 2, 3])
def test_loader_partition(packed_dir, world):
    _, out = packed_dir
    t = DeviceImageTransform(PreprocessCfg(size=32), is_train=True)
    loaders = [PackedLoader(out, 2, t, "cpu", world_size=world, rank=r, seed=5) for r in range(world)]
    assert len({l.num_batches for l in loaders}) == 1 and loaders[0].num_batches == (12 // world) // 2
    assert all(l.num_samples == 12 for l in loaders)
    for epoch in (0, 1):
        orders = [l.order(epoch) for l in loaders]
        flat = np.concatenate(orders)
        assert all(len(o) == loaders[0].num_batches * 2 for o in orders)
        assert len(set(flat.tolist())) == len(flat) and flat.min() >= 0 and flat.max() < 12      # disjoint ranks
    assert loaders[0].order(0).tolist() != loaders[0].order(1).tolist()
    assert loaders[0].order(0).tolist() == PackedLoader(out, 2, t, "cpu", world_size=world, rank=0, seed=5).order(0).tolist()
    with pytest.raises(ValueError, match="do not fill"):
        PackedLoader(out, 16, t, "cpu", world_size=world, rank=0)


def test_box_draw_is_a_function_of_seed_epoch_rank_batch(packed_dir):
    _, out = packed_dir
    t = DeviceImageTransform(PreprocessCfg(size=32), is_train=True, aug_cfg={"scale": (0.3, 1.0)})
    hw = torch.tensor([[60, 50]] * 32)

    def boxes(seed, epoch, rank, k, world=2):
        l = PackedLoader(out, 2, t, "cpu", world_size=world, rank=rank, seed=seed)
        return t.boxes(hw, l.batch_generator(epoch, k))

    base = boxes(5, 0, 0, 1)
    assert torch.equal(base, boxes(5, 0, 0, 1))
    for other in (boxes(6, 0, 0, 1), boxes(5, 1, 0, 1), boxes(5, 0, 1, 1), boxes(5, 0, 0, 2)):
        assert not torch.equal(base, other)
    # set_epoch reaches the loader through DataInfo
    from colxlip_amd.data import DataInfo
    l = PackedLoader(out, 2, t, "cpu", seed=5)
    DataInfo(dataloader=l).set_epoch(3)
    assert l.epoch == 3 and l.order().tolist() == l.order(3).tolist()
    plan = l.plan()
    assert len(plan) == l.num_batches and np.array_equal(np.concatenate([p[0] for p in plan]), l.order(3))


def test_get_data_packed(packed_dir):
    _, out = packed_dir
    assert parse_args(["--dataset-type", "packed"]).dataset_type == "packed"
    model, pre_t, pre_v = create_model_and_transforms("ViT-tiny-test", precision="fp32", device="cpu")
    args = parse_args(["--model", "ViT-tiny-test", "--dataset-type", "packed", "--train-data", out, "--batch-size", "4",
                       "--device", "cpu", "--workers", "2", "--aug-cfg", "scale=(0.5,1.0)"])
    args.rank, args.world_size = 0, 1
    data = get_data(args, (pre_t, pre_v), epoch=0)
    loader = data["train"].dataloader
    assert set(data) == {"train"} and loader.num_batches == 3 and loader.num_samples == 12
    assert loader.transform.size == tuple(model.visual.image_size) and loader.transform.scale == (0.5, 1.0)
    assert loader.transform.is_train and loader.transform.interpolation == "bicubic"
    args.aug_cfg = {"re_prob": 0.1}
    with pytest.raises(ValueError, match="re_prob"):
        get_data(args, (pre_t, pre_v))
    args.aug_cfg, args.train_data = {}, None
    with pytest.raises(ValueError):
        get_data(args, (pre_t, pre_v))
    args.retrieval_coco = True
    with pytest.raises(ValueError, match="val-data"):
        get_data(args, (pre_t, pre_v))
