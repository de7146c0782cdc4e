"""Generate the DistillClipLoss fixtures by running the reference's own `DistillClipLoss` (loss.py:343-379).

Like make_golden.py (whose helpers it imports), this runs only where the reference tree is available; the fixtures
are data only.  Every backward runs on `contrastive + DIST_W * distill`, so the two upstream gradients differ.

    python tests/golden/make_golden_distill.py [--loss-only]
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

DIST_W = 0.75
# (tag, b, Es, Et, log scale, teacher log scale, teacher needs grad): b = 100 is not a multiple of 64; (48, 96) is outside
# the fused embed dims (the materialising path); d has a teacher scale of 100 on aligned pairs (saturated teacher softmax);
# e gives the teacher features and scale a gradient
W1_CASES = (("a", 16, 64, 64, math.log(10.0), math.log(50.0), False),
            ("b", 100, 512, 768, 2.3, 3.5, False),
            ("c", 70, 48, 96, 1.7, 2.9, False),
            ("d", 40, 64, 64, math.log(20.0), math.log(100.0), False),
            ("e", 24, 64, 128, 2.0, 3.0, True))

SMALL = O.ClipCfg(embed_dim=64, image_size=64, patch_size=16, vision_width=128, vision_layers=2, context_length=77,
                  vocab_size=1024, text_width=128, text_heads=2, text_layers=2)          # tests/model_configs/ViT-small-test.json
TEACHER = O.ClipCfg(embed_dim=128, image_size=64, patch_size=16, vision_width=192, vision_layers=2, context_length=77,
                    vocab_size=1024, text_width=192, text_heads=3, text_layers=2)        # tests/model_configs/ViT-teacher-test.json


# the inputs of case b would take the fixture past 1 MB: the consumer regenerates them from their seed (checksummed)
SEEDED = ("b",)


def case_inputs(i, tag, b, es, et):
    """features of W1_CASES[i] from a per-case CPU generator (the consumer repeats this for the SEEDED cases)"""
    g = torch.Generator().manual_seed(21 + i)
    fi = F.normalize(torch.randn(b, es, generator=g), dim=-1)
    ft = F.normalize(torch.randn(b, es, generator=g), dim=-1)
    tfi = F.normalize(torch.randn(b, et, generator=g), dim=-1)
    tft = F.normalize(torch.randn(b, et, generator=g), dim=-1)
    if tag == "d":          # aligned teacher pairs at scale 100: the teacher softmax is one-hot to fp32 precision
        tft = F.normalize(tfi + 0.05 * tft, dim=-1)
    return fi, ft, tfi, tft


def golden_distill_loss(L):
    out = {}
    for i, (tag, b, es, et, ls0, tls0, tgrad) in enumerate(W1_CASES):
        fi, ft, tfi, tft = case_inputs(i, tag, b, es, et)
        leaves = [fi, ft] + ([tfi, tft] if tgrad else [])
        for x in leaves:
            x.requires_grad_(True)
        ls = torch.tensor(ls0).requires_grad_(True)
        tls = torch.tensor(tls0).requires_grad_(tgrad)
        c, d = L.DistillClipLoss()(fi, ft, ls.exp(), tfi, tft, tls.exp())
        (c + DIST_W * d).backward()
        p = f"{tag}/"
        feats = {p + "image_features": fi, p + "text_features": ft, p + "dist_image_features": tfi,
                 p + "dist_text_features": tft}
        if tag in SEEDED:
            out[p + "input_checksum"] = np.array([float(v.detach().double().sum()) for v in feats.values()])
        else:
            out.update(feats)
        out.update({p + "log_logit_scale": ls, p + "dist_log_logit_scale": tls, p + "contrastive_loss": c,
                    p + "distill_loss": d, p + "grad_image": fi.grad, p + "grad_text": ft.grad,
                    p + "grad_log_logit_scale": ls.grad})
        if tgrad:
            out.update({p + "grad_dist_image": tfi.grad, p + "grad_dist_text": tft.grad, p + "grad_dist_log_logit_scale": tls.grad})
    tl = math.exp(W1_CASES[3][5]) * (out["d/dist_image_features"].detach() @ out["d/dist_text_features"].detach().T)
    assert float(tl.softmax(1).diagonal().min()) > 0.999
    out["dist_w"] = np.array(DIST_W)
    save("distill_loss.npz", **out)


def _distill_dist_worker(rank, world, port, b, es, et, q):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    _, L = import_reference()
    g = torch.Generator().manual_seed(300 + rank)
    res = {}
    for local_loss in (False, True):
        for gwg in (False, True):
            fi = F.normalize(torch.randn(b, es, generator=g), dim=-1).requires_grad_(True)
            ft = F.normalize(torch.randn(b, es, generator=g), dim=-1).requires_grad_(True)
            tfi = F.normalize(torch.randn(b, et, generator=g), dim=-1)
            tft = F.normalize(torch.randn(b, et, generator=g), dim=-1)
            ls = torch.tensor(math.log(10.0) + 0.3).requires_grad_(True)
            tls = torch.tensor(math.log(30.0))
            loss = L.DistillClipLoss(local_loss=local_loss, gather_with_grad=gwg, rank=rank, world_size=world)
            c, d = loss(fi, ft, ls.exp(), tfi, tft, tls.exp())
            (c + DIST_W * d).backward()
            tag = f"w{world}/l{int(local_loss)}g{int(gwg)}/r{rank}"
            res.update({f"{tag}/image_features": fi.detach(), f"{tag}/text_features": ft.detach(),
                        f"{tag}/dist_image_features": tfi, f"{tag}/dist_text_features": tft,
                        f"{tag}/log_logit_scale": ls.detach(), f"{tag}/dist_log_logit_scale": tls,
                        f"{tag}/contrastive_loss": c.detach(), f"{tag}/distill_loss": d.detach(),
                        f"{tag}/grad_image": fi.grad, f"{tag}/grad_text": ft.grad, f"{tag}/grad_log_logit_scale": ls.grad})
            dist.barrier()
    q.put({k: v.numpy() for k, v in res.items()})
    dist.barrier()
    dist.destroy_process_group()


def golden_distill_dist():
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    allres = {}
    for world, port in ((2, 29631), (4, 29632)):
        q = ctx.Queue()
        procs = [ctx.Process(target=_distill_dist_worker, args=(r, world, port, 6, 16, 32, q)) for r in range(world)]
        for p in procs:
            p.start()
        for _ in range(world):
            allres.update(q.get())
        for p in procs:
            p.join()
    allres["dist_w"] = np.array(DIST_W)
    save("distill_dist.npz", **allres)


def _summary(grads):
    names = sorted(grads.keys())
    return {"grad_names": np.array(names),
            "grad_norms": np.array([float(grads[k].double().norm()) for k in names]),
            "grad_maxabs": np.array([float(grads[k].abs().max()) for k in names]),
            "grad_sample": np.stack([F.pad(grads[k].reshape(-1)[grad_sample_index(grads[k].numel())],
                                           (0, max(0, GRAD_SAMPLE - grads[k].numel()))).numpy() for k in names])}


def golden_distill_tiny(T, L):
    """ViT-small-test student + ViT-teacher-test teacher through the reference's towers and DistillClipLoss at batch 8.
    Weights and batch are regenerated from their seeds by the consumer (checksummed); features, both losses and the
    student's gradient summaries only (norm, largest magnitude, a strided sample of each gradient)."""
    sd = O.perturb_state_dict(O.init_state_dict(SMALL, seed=0), seed=1)
    tsd = O.perturb_state_dict(O.init_state_dict(TEACHER, seed=2), seed=3)
    image, text = O.synthetic_batch(SMALL, 8, seed=1234)
    vis, txt = build_ref_towers(T, SMALL, sd)
    tvis, ttxt = build_ref_towers(T, TEACHER, tsd)
    tvis.eval()
    ttxt.eval()
    logit_scale = torch.nn.Parameter(sd["logit_scale"].clone())
    with torch.no_grad():
        tfi = F.normalize(tvis(image), dim=-1)
        tft = F.normalize(ttxt(text), dim=-1)
    fi = F.normalize(vis(image), dim=-1)
    ft = F.normalize(txt(text), dim=-1)
    c, d = L.DistillClipLoss()(fi, ft, logit_scale.exp(), tfi, tft, tsd["logit_scale"].exp())
    (c + d).backward()
    grads = {"visual." + k: p.grad for k, p in vis.named_parameters()}
    grads.update({k: p.grad for k, p in txt.named_parameters()})
    grads["logit_scale"] = logit_scale.grad
    arrs = {"image_features": fi, "text_features": ft, "dist_image_features": tfi, "dist_text_features": tft,
            "contrastive_loss": c, "distill_loss": d, **_summary(grads),
            "sd_checksum": np.array([float(sd[k].double().sum()) for k in sorted(sd.keys())]),
            "teacher_checksum": np.array([float(tsd[k].double().sum()) for k in sorted(tsd.keys())]),
            "batch_checksum": np.array([float(image.double().sum()), float(text.double().sum())])}
    save("distill_tiny.npz", **arrs)


if __name__ == "__main__":
    torch.manual_seed(0)
    T, L = import_reference()
    golden_distill_loss(L)
    if "--loss-only" not in sys.argv:
        golden_distill_tiny(T, L)
        golden_distill_dist()
