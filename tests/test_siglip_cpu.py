"""SigLipLoss without a GPU: the flags, create_loss's branch order and refusals, no CPU fallback."""
import math
from types import SimpleNamespace

import pytest
import torch

from colxlip_amd import SigLipLoss
from colxlip_amd.factory import create_loss
from colxlip_amd.params import parse_args, unsupported_flag_values



def test_reference_import_path():
    from colxlip.loss import SigLipLoss as S, neighbour_exchange, neighbour_exchange_bidir  # noqa: F401
    from colxlip.loss import neighbour_exchange_with_grad, neighbour_exchange_bidir_with_grad  # noqa: F401
    assert S is SigLipLoss


def test_flags():
    a = parse_args(["--siglip", "--loss-dist-impl", "shift"])
    assert a.siglip and a.loss_dist_impl == "shift"
    assert unsupported_flag_values(a) == []
    assert parse_args([]).loss_dist_impl is None
    for impl in ("bidir", "shift", "reduce", "gather"):
        assert parse_args(["--loss-dist-impl", impl]).loss_dist_impl == impl
    with pytest.raises(SystemExit):
        parse_args(["--loss-dist-impl", "ring"])


def test_constructor_matches_reference_defaults():
    m = SigLipLoss()
    assert (m.cache_labels, m.rank, m.world_size, m.dist_impl) == (False, 0, 1, "bidir")
    assert SigLipLoss(dist_impl="gather", rank=1, world_size=4).dist_impl == "gather"
    with pytest.raises(AssertionError):
        SigLipLoss(dist_impl="ring")
    lab = m.get_ground_truth(torch.device("cpu"), torch.float32, 3)
    assert torch.equal(lab, 2 * torch.eye(3) - 1)
    assert torch.equal(m.get_ground_truth(torch.device("cpu"), torch.float32, 3, negative_only=True), -torch.ones(3, 3))


def _args(**kw):
    base = dict(model="ViT-B-32", siglip=False, horovod=False, distill_model=None, local_loss=False, gather_with_grad=False,
                rank=0, world_size=1, loss_dist_impl=None)
    base.update(kw)
    return SimpleNamespace(**base)


def test_create_loss_branch_order_and_refusals():
    loss = create_loss(_args(siglip=True, rank=1, world_size=4, loss_dist_impl="shift"))
    assert isinstance(loss, SigLipLoss) and (loss.rank, loss.world_size, loss.dist_impl) == (1, 4, "shift")
    assert create_loss(_args(siglip=True)).dist_impl == "bidir"
    with pytest.raises(NotImplementedError):                 # coca comes first, as in the reference
        create_loss(_args(model="coca_ViT-B-32", siglip=True))
    with pytest.raises(AssertionError):
        create_loss(_args(siglip=True, horovod=True))
    with pytest.raises(ValueError, match="ColXLIP"):
        create_loss(_args(model="ViT-B-16-colxlip", siglip=True))
    assert not isinstance(create_loss(_args()), SigLipLoss)


def test_no_cpu_fallback():
    fi = torch.nn.functional.normalize(torch.randn(8, 64), dim=-1).requires_grad_(True)
    ft = torch.nn.functional.normalize(torch.randn(8, 64), dim=-1)
    with pytest.raises(RuntimeError, match="device"):
        SigLipLoss()(fi, ft, torch.tensor(10.0), torch.tensor(-10.0))
    with torch.no_grad(), pytest.raises(RuntimeError, match="device"):
        SigLipLoss()(fi, ft, torch.tensor(math.log(10)), torch.tensor(-10.0))
