"""Generate the late-interaction retrieval fixture by running the reference's own `compute_colbert_similarity`
(loss.py:20-46) and `compute_retrieval` / `remap_indices` (train.py:429-508) on a non-square gallery.

Like make_golden.py (whose helpers it imports), this runs only where the reference tree is available; the fixture is
data only.  The scores are the scoring the reference's ColXLIP.forward carries as a commented-out block
(model.py:670-685), image-major: scale * (alpha * I T^T + (1 - alpha) * tok^T).

    python tests/golden/make_golden_late_interaction.py
"""
import ast
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from make_golden import REF, save  # noqa: E402

N_IMG, Q, N_TOK, E = 6, 16, 20, 32
CAPTIONS = (2, 1, 3, 1, 2, 1)            # captions per image: 10 in all
SCALE, ALPHA = 14.0, 0.7


def take(path, names):
    return [n for n in ast.parse(open(path).read()).body if isinstance(n, ast.FunctionDef) and n.name in names]


def main():
    ns = {"torch": torch, "np": np}
    exec(compile(ast.Module(body=take(REF + "/loss.py", ("compute_colbert_similarity",)), type_ignores=[]), REF + "/loss.py", "exec"), ns)
    exec(compile(ast.Module(body=take(REF + "/train.py", ("compute_retrieval", "remap_indices")), type_ignores=[]),
                 REF + "/train.py", "exec"), ns)
    g = torch.Generator().manual_seed(77)
    n_txt = sum(CAPTIONS)
    owner = torch.repeat_interleave(torch.arange(N_IMG), torch.tensor(CAPTIONS))
    fi = F.normalize(torch.randn(N_IMG, E, generator=g), dim=-1)
    ft = F.normalize(fi[owner] + 0.3 * torch.randn(n_txt, E, generator=g), dim=-1)                # aligned, noise norm ~1.7
    ti = F.normalize(torch.randn(N_IMG, Q, E, generator=g), dim=-1)
    tt = F.normalize(ti[owner][:, :1] + 0.3 * torch.randn(n_txt, N_TOK, E, generator=g), dim=-1)
    for m in range(n_txt):                 # ColXLIP's text tokens: one vector at and behind the EOT; sample 3 exact zeros there
        eot = 3 + (7 * m) % (N_TOK - 3)
        tt[m, eot:] = 0.0 if m == 3 else tt[m, eot].clone()
    tok = ns["compute_colbert_similarity"](ti, tt)                                                  # [n_txt, n_img]
    scores = SCALE * (ALPHA * fi @ ft.t() + (1 - ALPHA) * tok.t())
    img_ids = 300 + 11 * torch.randperm(N_IMG, generator=g)
    cap_ids = torch.arange(n_txt)
    img2txt = {int(img_ids[i]): [int(c) for c in cap_ids[owner == i]] for i in range(N_IMG)}
    txt2img = {int(c): [int(img_ids[owner[c]])] for c in range(n_txt)}
    new_i2t, new_t2i = ns["remap_indices"](merged_img_ids=img_ids, cap_ids=cap_ids, img2txt_dict=img2txt, txt2img_dict=txt2img)
    metrics = ns["compute_retrieval"](scores, new_t2i, new_i2t)
    save("late_interaction.npz", image_features=fi, text_features=ft, token_image_features=ti, token_text_features=tt,
         tok=tok, scores=scores, scale=np.array(SCALE), alpha=np.array(ALPHA), img_ids=img_ids, cap_ids=cap_ids,
         owner=owner, metric_names=np.array(list(metrics.keys())), metric_values=np.array([float(v) for v in metrics.values()]))


if __name__ == "__main__":
    main()
