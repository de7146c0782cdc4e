"""DistillClipLoss's four distributed forms (local_loss x gather_with_grad) on the MI355X: processes share the one GPU over
gloo (as tests/test_siglip_dist_gpu.py), so every rank runs the real gathers -- student and teacher features -- and the
kernels on the device.  Checked against the reference's DistillClipLoss over a gloo group (tests/golden/distill_dist.npz) on
every rank; then `main` with a teacher, --local-loss --gather-with-grad, as a 2-rank job."""
import os
import socket
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = ("l0g0", "l0g1", "l1g0", "l1g1")


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
    from colxlip_amd.loss import DistillClipLoss
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    z = np.load(os.path.join(ROOT, "tests", "golden", "distill_dist.npz"))
    w = float(z["dist_w"])
    res = {}
    for mode in MODES:
        tag = f"w{world}/{mode}/r{rank}"
        fi = torch.from_numpy(z[f"{tag}/image_features"]).cuda().requires_grad_(True)
        ft = torch.from_numpy(z[f"{tag}/text_features"]).cuda().requires_grad_(True)
        tfi = torch.from_numpy(z[f"{tag}/dist_image_features"]).cuda()
        tft = torch.from_numpy(z[f"{tag}/dist_text_features"]).cuda()
        ls = torch.from_numpy(z[f"{tag}/log_logit_scale"]).cuda().requires_grad_(True)
        tls = torch.from_numpy(z[f"{tag}/dist_log_logit_scale"]).cuda()
        loss = DistillClipLoss(local_loss=mode[1] == "1", gather_with_grad=mode[3] == "1", rank=rank, world_size=world)
        c, d = loss(fi, ft, ls.exp(), tfi, tft, tls.exp())
        (c + w * d).backward()
        res[mode] = {k: v.detach().cpu() for k, v in (("contrastive_loss", c), ("distill_loss", d), ("grad_image", fi.grad),
                                                      ("grad_text", ft.grad), ("grad_log_logit_scale", ls.grad))}
        dist.barrier()
    torch.save(res, os.path.join(out_dir, f"rank{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 4])
def test_dist_modes_vs_reference_fixture(tmp_path, world):
    import torch.multiprocessing as mp
    mp.spawn(_loss_worker, args=(world, _port(), str(tmp_path)), nprocs=world, join=True)
    z = np.load(os.path.join(ROOT, "tests", "golden", "distill_dist.npz"))
    for rank in range(world):
        got = torch.load(os.path.join(tmp_path, f"rank{rank}.pt"), weights_only=True)
        for mode in MODES:
            tag = f"w{world}/{mode}/r{rank}"
            g = got[mode]
            for key in ("contrastive_loss", "distill_loss", "grad_log_logit_scale"):
                want = float(z[f"{tag}/{key}"])
                assert abs(float(g[key]) - want) <= 1e-5 * abs(want) + 1e-7, (tag, key, float(g[key]), want)
            for key in ("grad_image", "grad_text"):
                want = torch.from_numpy(z[f"{tag}/{key}"])
                err = float((g[key] - want).abs().max())
                assert err <= 1e-5 * float(want.abs().max()), (tag, key, err)


def _runner_worker(rank, world, port, logs_dir, teacher_ckpt):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    from colxlip_amd import add_model_config
    from colxlip_amd import main as main_mod
    add_model_config(os.path.join(ROOT, "tests", "model_configs"))
    orig_close = main_mod._Run.close

    def close(self, clean=True):          # every rank leaves its final student weights behind
        if self.core is not None:
            torch.save({k: v.detach().cpu() for k, v in self.core.state_dict().items()},
                       os.path.join(logs_dir, f"final_rank{rank}.pt"))
        return orig_close(self, clean)

    main_mod._Run.close = close
    rc = main_mod.main(["--model", "ViT-small-test", "--dataset-type", "synthetic", "--precision", "fp32", "--batch-size", "8",
                        "--train-num-samples", str(8 * world * 3), "--epochs", "1", "--lr", "1e-3", "--lr-scheduler", "const",
                        "--warmup", "1", "--local-loss", "--gather-with-grad", "--distill-model", "ViT-teacher-test",
                        "--distill-pretrained", teacher_ckpt, "--logs-dir", logs_dir, "--name", "dist2", "--seed", "3",
                        "--log-every-n-steps", "1", "--dist-backend", "gloo", "--no-set-device-rank"])
    assert rc == 0


def test_runner_two_ranks_with_a_teacher(tmp_path):
    import torch.multiprocessing as mp
    sys.path.insert(0, ROOT)
    from oracle import clip_oracle as O
    teacher = O.ClipCfg(embed_dim=128, image_size=64, patch_size=16, vision_width=192, vision_layers=2, context_length=77,
                        vocab_size=1024, text_width=192, text_heads=3, text_layers=2)
    ckpt = str(tmp_path / "teacher.pt")
    torch.save(O.perturb_state_dict(O.init_state_dict(teacher, seed=2), seed=3), ckpt)
    mp.spawn(_runner_worker, args=(2, _port(), str(tmp_path), ckpt), nprocs=2, join=True)
    w0 = torch.load(os.path.join(tmp_path, "final_rank0.pt"), weights_only=True)
    w1 = torch.load(os.path.join(tmp_path, "final_rank1.pt"), weights_only=True)
    ck = torch.load(os.path.join(tmp_path, "dist2", "checkpoints", "epoch_1.pt"), map_location="cpu", weights_only=True)
    sd = {k[len("module."):] if k.startswith("module.") else k: v for k, v in ck["state_dict"].items()}
    assert set(w0) == set(w1) == set(sd)
    for k in w0:
        assert torch.equal(w0[k], w1[k]), k
        assert not w0[k].is_floating_point() or torch.isfinite(w0[k]).all(), k
