"""Patch dropout without a GPU: the kept-token count of the reference (transformer.py:76-77, Python float), the probability check,
ColXLIP's refusal, that the control object adds nothing to the state dict, and that the `rng="torch"` draw replays the masks the
reference drew for tests/golden/patch_dropout.npz (written by make_golden_patch_dropout.py)."""
import os

import numpy as np
import pytest
import torch

import colxlip_amd
from colxlip_amd.model import PatchDropout

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "patch_dropout.npz")


@pytest.mark.parametrize("G2", [4, 10, 16, 20, 49, 196, 256, 576])
@pytest.mark.parametrize("p", [0.0, 0.1, 0.25, 0.3, 0.5, 0.6, 0.7, 0.75, 0.8, 0.9, 0.95, 0.99])
def test_num_keep_matches_the_reference(G2, p):
    assert PatchDropout(p).num_keep(G2) == max(1, int(G2 * (1 - p)))


def test_num_keep_rounds_like_python_float():
    assert PatchDropout(0.9).num_keep(20) == 1            # 20 * (1 - 0.9) = 1.9999999999999996
    assert PatchDropout(0.5).num_keep(49) == 24
    assert PatchDropout(0.75).num_keep(49) == 12
    assert PatchDropout(0.5).num_keep(196) == 98


@pytest.mark.parametrize("p", [-0.1, 1.0, 1.5])
def test_probability_outside_unit_interval_raises(p):
    with pytest.raises(ValueError):
        PatchDropout(p)
    with pytest.raises(ValueError):
        colxlip_amd.create_model("ViT-small-test", force_patch_dropout=p)


def test_rng_and_first_token_options():
    with pytest.raises(ValueError):
        PatchDropout(0.5, rng="numpy")
    with pytest.raises(NotImplementedError):
        PatchDropout(0.5, exclude_first_token=False)
    pd = PatchDropout(0.5)
    assert pd.rng == "device" and pd.last_keep_index is None
    pd.rng = "torch"
    assert pd.rng == "torch"
    with pytest.raises(AttributeError):
        pd.last_keep_index = torch.zeros(1)


def test_model_with_patch_dropout_builds_and_keeps_its_state_dict():
    m0 = colxlip_amd.create_model("ViT-small-test")
    m = colxlip_amd.create_model("ViT-small-test", force_patch_dropout=0.5)
    assert m.visual.patch_dropout.prob == 0.5 and m0.visual.patch_dropout.prob == 0.0
    assert list(m.state_dict()) == list(m0.state_dict())
    assert [n for n, _ in m.named_parameters()] == [n for n, _ in m0.named_parameters()]
    assert not list(m.visual.patch_dropout.parameters()) and not list(m.visual.patch_dropout.buffers())
    m.eval()
    assert not m.visual.patch_dropout.training


def test_colxlip_refuses_patch_dropout():
    with pytest.raises(NotImplementedError, match="ColXLIP"):
        colxlip_amd.create_model("ViT-small-test-colxlip", force_patch_dropout=0.5)
    colxlip_amd.create_model("ViT-small-test-colxlip", force_patch_dropout=0.0)


def _cases():
    z = np.load(GOLDEN)
    return sorted({k.split("/")[0] for k in z.files})


@pytest.mark.parametrize("tag", _cases())
def test_torch_rng_replays_the_reference_masks(tag):
    z = np.load(GOLDEN)
    prob, seed, batch = float(z[f"{tag}/prob"]), int(z[f"{tag}/seed"]), int(z[f"{tag}/batch"])
    want = z[f"{tag}/keep_index"]
    G2 = {"small": 16, "b16": 196}[tag.split("_")[0]]
    pd = PatchDropout(prob, rng="torch")
    assert want.shape == (batch, pd.num_keep(G2))
    torch.manual_seed(seed)
    got = pd.draw(batch, G2, "cpu")
    assert got.dtype == torch.int32
    assert np.array_equal(got.numpy().astype(np.int64), want)
