"""DistillClipLoss without a GPU: the import path and constructor, the flags, create_loss's branch, main's refusals (they
read only flags and model configs), no CPU fallback."""
import os
from types import SimpleNamespace

import pytest
import torch

from colxlip_amd import ClipLoss, DistillClipLoss, SigLipLoss
from colxlip_amd.factory import create_loss
from colxlip_amd.main import distill_refusal
from colxlip_amd.params import parse_args, unsupported_flag_values

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_reference_import_path():
    from colxlip.loss import DistillClipLoss as D
    assert D is DistillClipLoss and issubclass(D, ClipLoss)


def test_constructor_matches_reference_defaults():
    m = DistillClipLoss()
    assert (m.local_loss, m.gather_with_grad, m.cache_labels, m.rank, m.world_size, m.use_horovod) == \
        (False, False, False, 0, 1, False)
    m = DistillClipLoss(local_loss=True, gather_with_grad=True, cache_labels=True, rank=1, world_size=2)
    assert (m.local_loss, m.gather_with_grad, m.cache_labels, m.rank, m.world_size) == (True, True, True, 1, 2)
    assert torch.equal(m.get_ground_truth(torch.device("cpu"), 3), torch.arange(3) + 3)    # inherited, offset by rank
    assert DistillClipLoss.get_logits is ClipLoss.get_logits


def test_flags():
    a = parse_args(["--distill-model", "ViT-B-16", "--distill-pretrained", "/tmp/t.pt"])
    assert (a.distill_model, a.distill_pretrained) == ("ViT-B-16", "/tmp/t.pt")
    assert unsupported_flag_values(a) == []
    assert unsupported_flag_values(parse_args(["--distill-model", "ViT-B-16"])) == []
    b = parse_args([])
    assert b.distill_model is None and b.distill_pretrained is None


def _args(**kw):
    base = dict(model="ViT-B-32", siglip=False, horovod=False, distill_model=None, distill_pretrained=None, local_loss=False,
                gather_with_grad=False, rank=0, world_size=1, loss_dist_impl=None)
    base.update(kw)
    return SimpleNamespace(**base)


def test_create_loss_returns_distill_loss():
    loss = create_loss(_args(distill_model="ViT-B-16", distill_pretrained="t.pt", rank=1, world_size=4, local_loss=True,
                             gather_with_grad=True))
    assert isinstance(loss, DistillClipLoss)
    assert (loss.rank, loss.world_size, loss.local_loss, loss.gather_with_grad, loss.cache_labels) == (1, 4, True, True, True)
    # one flag alone does not switch distillation on (main refuses it); the flag-less namespace of older callers still works
    assert type(create_loss(_args(distill_model="ViT-B-16"))) is ClipLoss
    assert type(create_loss(_args(distill_pretrained="t.pt"))) is ClipLoss
    ns = SimpleNamespace(model="ViT-B-32", siglip=False, horovod=False, distill_model=None, local_loss=False,
                         gather_with_grad=False, rank=0, world_size=1)
    assert type(create_loss(ns)) is ClipLoss


def test_create_loss_refusals_and_order():
    on = dict(distill_model="ViT-B-16", distill_pretrained="t.pt")
    with pytest.raises(NotImplementedError):                 # coca comes first, as in the reference
        create_loss(_args(model="coca_ViT-B-32", **on))
    assert isinstance(create_loss(_args(siglip=True, **on)), SigLipLoss)      # then siglip
    with pytest.raises(ValueError, match="ColXLIP"):
        create_loss(_args(model="ViT-B-16-colxlip", **on))


def _main_args(*extra):
    from colxlip_amd import add_model_config
    add_model_config(os.path.join(ROOT, "tests", "model_configs"))
    return parse_args(["--model", "ViT-small-test", *extra])


def test_main_refuses_a_teacher_with_another_context_length(tmp_path):
    import json
    from colxlip_amd import add_model_config, get_model_config
    cfg = get_model_config("ViT-teacher-test") or json.load(open(os.path.join(ROOT, "tests", "model_configs",
                                                                               "ViT-teacher-test.json")))
    cfg["text_cfg"]["context_length"] = 32
    (tmp_path / "ViT-teacher-ctx32-test.json").write_text(json.dumps(cfg))
    add_model_config(str(tmp_path))
    why = distill_refusal(_main_args("--distill-model", "ViT-teacher-ctx32-test", "--distill-pretrained", "t.pt"))
    assert "context length" in why


def test_main_refusals():
    ok = ("--distill-model", "ViT-teacher-test", "--distill-pretrained", "t.pt")
    assert distill_refusal(_main_args()) is None
    assert distill_refusal(_main_args(*ok)) is None
    assert "both" in distill_refusal(_main_args("--distill-model", "ViT-teacher-test"))
    assert "both" in distill_refusal(_main_args("--distill-pretrained", "t.pt"))
    assert "accum-freq" in distill_refusal(_main_args(*ok, "--accum-freq", "2"))
    assert "siglip" in distill_refusal(_main_args(*ok, "--siglip"))
    assert "ColXLIP" in distill_refusal(_main_args("--distill-model", "ViT-small-test-colxlip", "--distill-pretrained", "t.pt"))
    assert "ColXLIP" in distill_refusal(parse_args(["--model", "ViT-small-test-colxlip", *ok]))
    assert "CoCa" in distill_refusal(_main_args("--distill-model", "coca_ViT-B-32", "--distill-pretrained", "t.pt"))
    assert "image size" in distill_refusal(_main_args("--distill-model", "ViT-B-16", "--distill-pretrained", "t.pt"))
    assert "vocabulary" in distill_refusal(_main_args(*ok, "--model", "ViT-tiny-test", "--force-image-size", "64"))
    assert "not found" in distill_refusal(_main_args("--distill-model", "ViT-nonexistent", "--distill-pretrained", "t.pt"))


def test_no_cpu_fallback():
    fi = torch.nn.functional.normalize(torch.randn(8, 64), dim=-1).requires_grad_(True)
    ft = torch.nn.functional.normalize(torch.randn(8, 64), dim=-1)
    tfi = torch.nn.functional.normalize(torch.randn(8, 128), dim=-1)
    tft = torch.nn.functional.normalize(torch.randn(8, 128), dim=-1)
    with pytest.raises(RuntimeError, match="device"):
        DistillClipLoss()(fi, ft, torch.tensor(10.0), tfi, tft, torch.tensor(30.0))
    with torch.no_grad(), pytest.raises(RuntimeError, match="device"):
        DistillClipLoss()(fi, ft, torch.tensor(10.0), tfi[:, :48], tft[:, :48], torch.tensor(30.0))
