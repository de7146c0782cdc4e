"""SigLipLoss's four distributed forms on the MI355X: processes share the one GPU over gloo (as tests/test_two_ranks_gpu.py),
so every rank runs the real exchange code -- the ring's host-staged point-to-point rounds, the gather's all-gather and its
reduce-scatter backward -- and its kernels on the device.  Checked against the reference's SigLipLoss over a gloo group
(tests/golden/siglip_dist.npz) on every rank; then `main --siglip --loss-dist-impl shift` as a 2-rank job."""
import os
import socket
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IMPLS = ("bidir", "shift", "reduce", "gather")


def _port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _loss_worker(rank, world, port, out_dir):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch.distributed as dist
    from colxlip_amd.loss import SigLipLoss
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    z = np.load(os.path.join(ROOT, "tests", "golden", "siglip_dist.npz"))
    res = {}
    for impl in IMPLS:
        tag = f"w{world}/{impl}/r{rank}"
        fi = torch.from_numpy(z[f"{tag}/image_features"]).cuda().requires_grad_(True)
        ft = torch.from_numpy(z[f"{tag}/text_features"]).cuda().requires_grad_(True)
        ls = torch.from_numpy(z[f"{tag}/log_logit_scale"]).cuda().requires_grad_(True)
        lb = torch.from_numpy(z[f"{tag}/logit_bias"]).cuda().requires_grad_(True)
        loss = SigLipLoss(rank=rank, world_size=world, dist_impl=impl)(fi, ft, ls.exp(), lb)
        loss.backward()
        res[impl] = {k: v.detach().cpu() for k, v in (("loss", loss), ("grad_image", fi.grad), ("grad_text", ft.grad),
                                                      ("grad_log_logit_scale", ls.grad), ("grad_logit_bias", lb.grad))}
        with torch.no_grad():
            res[impl]["loss_nograd"] = SigLipLoss(rank=rank, world_size=world, dist_impl=impl)(fi, ft, ls.exp(), lb).cpu()
        dist.barrier()
    torch.save(res, os.path.join(out_dir, f"rank{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 4])
def test_dist_impls_vs_reference_fixture(tmp_path, world):
    import torch.multiprocessing as mp
    mp.spawn(_loss_worker, args=(world, _port(), str(tmp_path)), nprocs=world, join=True)
    z = np.load(os.path.join(ROOT, "tests", "golden", "siglip_dist.npz"))
    for rank in range(world):
        got = torch.load(os.path.join(tmp_path, f"rank{rank}.pt"), weights_only=True)
        for impl in IMPLS:
            tag = f"w{world}/{impl}/r{rank}"
            g = got[impl]
            for key in ("loss", "grad_log_logit_scale", "grad_logit_bias"):
                want = float(z[f"{tag}/{key}"])
                assert abs(float(g[key]) - want) <= 1e-5 * abs(want) + 1e-7, (tag, key, float(g[key]), want)
            assert abs(float(g["loss_nograd"]) - float(z[f"{tag}/loss"])) <= 1e-5 * abs(float(z[f"{tag}/loss"]))
            for key in ("grad_image", "grad_text"):
                want = torch.from_numpy(z[f"{tag}/{key}"])
                err = float((g[key] - want).abs().max())
                assert err <= 1e-5 * float(want.abs().max()), (tag, key, err)


def _runner_worker(rank, world, port, logs_dir):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    from colxlip_amd import add_model_config
    from colxlip_amd.main import main
    add_model_config(os.path.join(ROOT, "tests", "model_configs"))
    rc = main(["--model", "ViT-small-test", "--dataset-type", "synthetic", "--precision", "fp32", "--batch-size", "8",
               "--train-num-samples", str(8 * world * 3), "--epochs", "1", "--lr", "1e-3", "--lr-scheduler", "const",
               "--warmup", "1", "--siglip", "--loss-dist-impl", "shift", "--logs-dir", logs_dir, "--name", "sig2", "--seed", "3",
               "--log-every-n-steps", "1", "--dist-backend", "gloo", "--no-set-device-rank"])
    assert rc == 0


def test_runner_two_ranks_siglip_shift(tmp_path):
    import math
    import torch.multiprocessing as mp
    mp.spawn(_runner_worker, args=(2, _port(), str(tmp_path)), nprocs=2, join=True)
    ck = torch.load(os.path.join(tmp_path, "sig2", "checkpoints", "epoch_1.pt"), map_location="cpu", weights_only=True)
    sd = {k[len("module."):] if k.startswith("module.") else k: v for k, v in ck["state_dict"].items()}
    bias = float(sd["logit_bias"])
    assert math.isfinite(bias) and bias != -10.0
    assert all(torch.isfinite(v).all() for v in sd.values() if v.is_floating_point())
