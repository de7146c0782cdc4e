"""Generate the SigLipLoss fixtures by running the reference's own `SigLipLoss` (loss.py:470-604).

Like make_golden.py (whose helpers it imports), this runs only where the reference tree is available; the fixtures
are data only.

    python tests/golden/make_golden_siglip.py
"""
import math
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from make_golden import GRAD_SAMPLE, O, build_ref_towers, grad_sample_index, import_reference, save  # noqa: E402

# (tag, b, E, log scale, bias): b not a multiple of 64, a fused embed dim (64, 512) and one that is not (48); the last rows
# have s = 100, beta = -10 so |z| passes 88 (exp overflows in fp32 there)
W1_CASES = (("a", 16, 64, math.log(10.0), -10.0), ("b", 100, 512, 2.3, -3.0), ("c", 70, 48, 1.7, 0.5),
            ("d", 40, 64, math.log(100.0), -10.0))


def golden_siglip_loss(L):
    g = torch.Generator().manual_seed(11)
    out = {}
    for tag, b, e, ls0, lb0 in W1_CASES:
        fi = F.normalize(torch.randn(b, e, generator=g), dim=-1)
        ft = F.normalize(torch.randn(b, e, generator=g), dim=-1)
        if tag == "d":          # aligned pairs: positives at z ~ +90, so both tails of the softplus are hit
            ft = F.normalize(fi + 0.05 * ft, dim=-1)
        fi.requires_grad_(True)
        ft.requires_grad_(True)
        ls = torch.tensor(ls0).requires_grad_(True)
        lb = torch.tensor(lb0).requires_grad_(True)
        loss = L.SigLipLoss()(fi, ft, ls.exp(), lb)
        loss.backward()
        zmax = float((ls.exp() * fi @ ft.T + lb).abs().max())
        out.update({f"{tag}/image_features": fi, f"{tag}/text_features": ft, f"{tag}/log_logit_scale": ls,
                    f"{tag}/logit_bias": lb, f"{tag}/loss": loss, f"{tag}/grad_image": fi.grad, f"{tag}/grad_text": ft.grad,
                    f"{tag}/grad_log_logit_scale": ls.grad, f"{tag}/grad_logit_bias": lb.grad, f"{tag}/max_abs_z": zmax})
    assert out["d/max_abs_z"] > 88
    save("siglip_loss.npz", **out)


def _siglip_dist_worker(rank, world, port, b, e, q):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    _, L = import_reference()
    g = torch.Generator().manual_seed(200 + rank)
    res = {}
    for impl in ("bidir", "shift", "reduce", "gather"):
        fi = F.normalize(torch.randn(b, e, generator=g), dim=-1).requires_grad_(True)
        ft = F.normalize(torch.randn(b, e, generator=g), dim=-1).requires_grad_(True)
        ls = torch.tensor(math.log(10.0) + 0.2).requires_grad_(True)
        lb = torch.tensor(-8.0).requires_grad_(True)
        loss = L.SigLipLoss(rank=rank, world_size=world, dist_impl=impl)(fi, ft, ls.exp(), lb)
        loss.backward()
        tag = f"w{world}/{impl}/r{rank}"
        res.update({f"{tag}/image_features": fi.detach(), f"{tag}/text_features": ft.detach(), f"{tag}/loss": loss.detach(),
                    f"{tag}/grad_image": fi.grad, f"{tag}/grad_text": ft.grad, f"{tag}/log_logit_scale": ls.detach(),
                    f"{tag}/logit_bias": lb.detach(), f"{tag}/grad_log_logit_scale": ls.grad, f"{tag}/grad_logit_bias": lb.grad})
        dist.barrier()
    q.put({k: v.numpy() for k, v in res.items()})
    dist.barrier()
    dist.destroy_process_group()


def golden_siglip_dist():
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    allres = {}
    for world, port in ((2, 29621), (4, 29622)):
        q = ctx.Queue()
        procs = [ctx.Process(target=_siglip_dist_worker, args=(r, world, port, 6, 16, q)) for r in range(world)]
        for p in procs:
            p.start()
        for _ in range(world):
            allres.update(q.get())
        for p in procs:
            p.join()
    save("siglip_dist.npz", **allres)


def golden_siglip_tiny(T, L):
    """tiny_clip.npz's model and batch with a logit bias (-10, open_clip's SigLIP start) and the reference's SigLipLoss.
    Weights and batch are regenerated from their seeds by the consumer (checksummed); features, loss and gradient summaries
    only: every gradient's norm and largest magnitude, and a strided sample of its elements."""
    cfg = O.TINY
    sd = O.perturb_state_dict(O.init_state_dict(cfg, seed=0), seed=1)
    sd["logit_bias"] = torch.tensor(-10.0)
    image, text = O.synthetic_batch(cfg, 8, seed=1234)
    vis, txt = build_ref_towers(T, cfg, {k: v for k, v in sd.items() if k != "logit_bias"})
    logit_scale = torch.nn.Parameter(sd["logit_scale"].clone())
    logit_bias = torch.nn.Parameter(sd["logit_bias"].clone())
    fi = F.normalize(vis(image), dim=-1)
    ft = F.normalize(txt(text), dim=-1)
    loss = L.SigLipLoss()(fi, ft, logit_scale.exp(), logit_bias)
    loss.backward()
    grads = {"visual." + k: p.grad for k, p in vis.named_parameters()}
    grads.update({k: p.grad for k, p in txt.named_parameters()})
    grads["logit_scale"] = logit_scale.grad
    grads["logit_bias"] = logit_bias.grad
    names = sorted(grads.keys())
    arrs = {"image_features": fi, "text_features": ft, "loss": loss, "grad_names": np.array(names),
            "grad_norms": np.array([float(grads[k].double().norm()) for k in names]),
            "grad_maxabs": np.array([float(grads[k].abs().max()) for k in names]),
            "grad_sample": np.stack([F.pad(grads[k].reshape(-1)[grad_sample_index(grads[k].numel())],
                                           (0, max(0, GRAD_SAMPLE - grads[k].numel()))).numpy() for k in names]),
            "sd_checksum": np.array([float(sd[k].double().sum()) for k in sorted(sd.keys())]),
            "batch_checksum": np.array([float(image.double().sum()), float(text.double().sum())])}
    save("siglip_tiny.npz", **arrs)


if __name__ == "__main__":
    torch.manual_seed(0)
    T, L = import_reference()
    golden_siglip_loss(L)
    golden_siglip_tiny(T, L)
    golden_siglip_dist()
