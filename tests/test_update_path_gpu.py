"""The kernels that end every training step, each against a plain reference (tests/update_path_ref.py): multi-tensor and
single-tensor AdamW, FusedAdamW end to end, the bf16 and e4m3 weight refresh (per tensor, multi-tensor, and through the
engines' own descriptor packers), the flat gradient casts, sumsq and the two scale kernels."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from colxlip_amd import ops  # noqa: E402
from colxlip_amd._lib import ClipxError  # noqa: E402
from colxlip_amd.optim import FusedAdamW, param_groups  # noqa: E402
from tests import update_path_ref as R  # noqa: E402

DEV = "cuda"
B1, B2 = R.BETAS


def relerr(a, b):
    a, b = a.detach().float(), b.detach().float()
    return float((a - b).abs().max() / (b.abs().max() + 1e-12))


def bits(t):
    """the tensor's bytes as integers, for bit-for-bit comparisons (-0 != +0, NaN payloads count)"""
    return t.contiguous().view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()])


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(bits(a), bits(b))


# ------------------------------------------------------------------------------------------------ AdamW
def _packer():
    return FusedAdamW([torch.nn.Parameter(torch.zeros(1, device=DEV))])


def _check_adamw(got, ref, label):
    """p, m, v within ADAMW_TOL_* x 2^-24 x magnitude sum of adamw_ref, element by element; prints the worst ratio to the bound"""
    dev = R.adamw_deviation(got, ref)
    ratio = [d / t for d, t in zip(dev, (R.ADAMW_TOL_P, R.ADAMW_TOL_M, R.ADAMW_TOL_V))]
    print(f"[adamw] {label}: deviation / bound  p {ratio[0]:.3g}  m {ratio[1]:.3g}  v {ratio[2]:.3g}")
    bad = [int((~ok).sum()) for ok in R.adamw_within(got, ref)]
    assert bad == [0, 0, 0], f"{label}: elements outside the bound (p, m, v) {bad}; deviation / bound {ratio}"


def _launch_over_arenas(layout, cpu_arenas, lr, step, gscale, label):
    arenas = [a.to(DEV) for a in cpu_arenas]
    before = [a.clone() for a in arenas]
    assert all(a.data_ptr() % 16 == 0 for a in arenas)
    entries = R.arena_views(arenas, layout)
    table, blocks = _packer()._multi_table(entries)
    assert blocks == sum((n + R.ADAMW_BLOCK - 1) // R.ADAMW_BLOCK for n, _, _ in layout)
    ops.adamw_multi(table, len(entries), blocks, lr, B1, B2, R.EPS, step, gscale)
    torch.cuda.synchronize()
    ref = R.adamw_ref(*R.gather(before, layout), lr, B1, B2, R.EPS, R.wd_vector(layout).to(DEV), step, gscale)
    p1, g1, m1, v1 = R.gather(arenas, layout)
    _check_adamw((p1, m1, v1), ref, label)
    assert same_bits(arenas[1], before[1]), f"{label}: the gradient arena was written"
    for s in (0, 2, 3):
        guard = R.guard_mask(layout, arenas[s].numel(), s).to(DEV)
        assert same_bits(arenas[s][guard], before[s][guard]), f"{label}: a guard element of stream {s} was written"
        assert bool((before[s][guard] == R.SENTINEL).all())


@pytest.mark.parametrize("name,lr,step,gscale", R.MIXED_RUNS, ids=[r[0] for r in R.MIXED_RUNS])
def test_adamw_multi_mixed_sizes_and_alignments(name, lr, step, gscale):
    """clipx_adamw_multi, one launch over 27 views into four flat arenas: sizes around the 4096-element block (1 ... 3 * 4096 +
    1023), each 16-byte aligned in all streams (vector body + scalar tail), with only p off by one element and with only v off
    by two (one misaligned stream sends the whole tensor down the scalar path), weight decay alternating 0 / 0.2, sentinel
    guards between neighbours.  The table comes from FusedAdamW._multi_table, so its record layout is checked against
    struct AdamwDesc too."""
    layout, _, cpu_arenas = R.mixed_arenas()
    _launch_over_arenas(layout, cpu_arenas, lr, step, gscale, name)


def test_adamw_multi_301_tensors():
    """301 tensors (a non-power-of-two count for the binary search over block0, ViT-B/32 has 302), sizes 1..5000, tensor i with
    weight decay 0.001 i at lr 1e-2: a block attributed to a neighbour reads the neighbour's record."""
    layout, _, cpu_arenas = R.many_arenas()
    name, lr, step, gscale = R.MANY_RUN
    _launch_over_arenas(layout, cpu_arenas, lr, step, gscale, name)


def test_adamw_multi_one_tensor():
    name, lr, step, gscale = R.SINGLE_RUN
    p, g, m, v = (t.to(DEV) for t in R.single_values())
    before = [t.clone() for t in (p, g, m, v)]
    table, blocks = _packer()._multi_table([(p, g, m, v, R.SINGLE_WD)])
    assert blocks == 2
    ops.adamw_multi(table, 1, blocks, lr, B1, B2, R.EPS, step, gscale)
    _check_adamw((p, m, v), R.adamw_ref(*before, lr, B1, B2, R.EPS, R.SINGLE_WD, step, gscale), name)
    assert same_bits(g, before[1])


def test_adamw_single_tensor_past_grid_cap():
    """clipx_adamw at n = 4 * 256 * 4096 + 4 * 256 + 3: more 16-byte groups than the 4096-block grid holds (the grid-stride
    loop wraps) and an n & 3 tail, with sentinels behind the end."""
    name, lr, step, gscale = R.CAP_RUN
    n = R.CAP_N
    bufs = [torch.full((n + 5,), R.SENTINEL, device=DEV) for _ in range(4)]
    for b, x in zip(bufs, R.cap_values()):
        b[:n] = x.to(DEV)
    before = [b.clone() for b in bufs]
    p, g, m, v = (b[:n] for b in bufs)
    ops.adamw(p, g, m, v, lr, B1, B2, R.EPS, R.CAP_WD, step, gscale)
    ref = R.adamw_ref(*(b[:n] for b in before), lr, B1, B2, R.EPS, R.CAP_WD, step, gscale)
    _check_adamw((p, m, v), ref, name)
    assert same_bits(bufs[1], before[1])
    assert all(same_bits(b[n:], o[n:]) for b, o in zip(bufs, before))


E2E_SHAPES = tuple((n,) for n in R.MIXED_SIZES) + ((33, 31), (64, 64), (100, 72))


def _e2e_grads(step, scale=1.0):
    gen = torch.Generator().manual_seed(100 + step)
    return [(torch.randn(*s, generator=gen) * 10.0 ** (i % 3 - 1) * scale).to(DEV) for i, s in enumerate(E2E_SHAPES)]


def _e2e_pair():
    gen = torch.Generator().manual_seed(7)
    init = [torch.randn(*s, generator=gen) for s in E2E_SHAPES]
    ours = [torch.nn.Parameter(t.clone().to(DEV)) for t in init]
    theirs = [torch.nn.Parameter(t.clone().to(DEV)) for t in init]
    groups = lambda ps: [{"params": ps[0::2], "weight_decay": 0.0}, {"params": ps[1::2], "weight_decay": 0.2}]   # noqa: E731
    opt = FusedAdamW(groups(ours), lr=5e-4, betas=R.BETAS, eps=R.EPS)
    ref = torch.optim.AdamW(groups(theirs), lr=5e-4, betas=R.BETAS, eps=R.EPS)
    return ours, theirs, opt, ref


def _e2e_compare(ours, theirs, opt, ref, label):
    for i, (p, q) in enumerate(zip(ours, theirs)):
        assert relerr(p, q) < 1e-6, (label, i, relerr(p, q))
        if p in opt.state and "exp_avg" in opt.state[p]:
            # torch rounds the doubles 1 - beta to fp32 (0.1f, 0.02f), the kernel forms 1.0f - beta: 9 resp. 49 units of 2^-24
            # apart (tests/test_update_path_cpu.py), plus a few roundings
            assert relerr(opt.state[p]["exp_avg"], ref.state[q]["exp_avg"]) < 16 * R.U32, (label, i)
            assert relerr(opt.state[p]["exp_avg_sq"], ref.state[q]["exp_avg_sq"]) < 64 * R.U32, (label, i)
            assert int(opt.state[p]["step"]) == int(ref.state[q]["step"]), (label, i)


def _count_calls(monkeypatch):
    calls = {"multi": 0, "single": 0}
    multi, single = ops.adamw_multi, ops.adamw

    def adamw_multi(*a, **k):
        calls["multi"] += 1
        return multi(*a, **k)

    def adamw(*a, **k):
        calls["single"] += 1
        return single(*a, **k)
    monkeypatch.setattr(ops, "adamw_multi", adamw_multi)
    monkeypatch.setattr(ops, "adamw", adamw)
    return calls


def test_fused_adamw_follows_torch_adamw(monkeypatch):
    """FusedAdamW against torch.optim.AdamW (fp32, on the device) over four steps on twelve parameters in two groups: the
    cached fast path (step 2), new gradient tensors at new addresses (step 3: the cached entry and the device table must go,
    the update must read the new gradient), load_state_dict(state_dict()) (before step 4) and a grad_scale."""
    calls = _count_calls(monkeypatch)
    ours, theirs, opt, ref = _e2e_pair()
    keep = []
    for step in (1, 2, 3, 4):
        gscale = 0.5 if step == 4 else 1.0                           # a power of two: the pre-scaled reference gradient is exact
        grads = _e2e_grads(step)
        for p, q, g in zip(ours, theirs, grads):
            if step == 2:
                p.grad.copy_(g)                                      # same storage as at step 1: the steady state
            else:
                keep.append(p.grad)                                  # keeps the old storage alive, so the new address differs
                p.grad = g.clone()
                assert keep[-1] is None or p.grad.data_ptr() != keep[-1].data_ptr()
            q.grad = g * gscale
        versions = [p._version for p in ours]
        fast_before = getattr(opt, "_fast", None)
        opt.step(grad_scale=gscale)
        ref.step()
        assert all(p._version > v0 for p, v0 in zip(ours, versions)), step
        _e2e_compare(ours, theirs, opt, ref, f"step {step}")
        if step == 2:
            assert fast_before is not None and opt._fast is fast_before        # the cached entry was used ...
        if step == 3:
            assert opt._fast is not fast_before                                  # ... and dropped when the gradients moved
            opt.load_state_dict(opt.state_dict())
            assert opt._fast is None
    assert calls == {"multi": 4, "single": 0}


def test_fused_adamw_mixed_step_counts_fall_back_per_tensor(monkeypatch):
    """One parameter gets its first gradient only at step 3: the step counts are mixed from then on and every tensor goes
    through clipx_adamw (the per-tensor fallback) with its own bias correction."""
    calls = _count_calls(monkeypatch)
    ours, theirs, opt, ref = _e2e_pair()
    late = 5                                                         # the 4097-element vector
    for step in (1, 2, 3, 4):
        for i, (p, q, g) in enumerate(zip(ours, theirs, _e2e_grads(step))):
            if i == late and step < 3:
                continue
            p.grad, q.grad = g.clone(), g.clone()
        versions = [p._version for p in ours]
        opt.step()
        ref.step()
        for i, (p, v0) in enumerate(zip(ours, versions)):
            assert (p._version > v0) == (i != late or step >= 3), (step, i)
        _e2e_compare(ours, theirs, opt, ref, f"step {step}")
        if step == 2:
            assert calls == {"multi": 2, "single": 0}
    assert calls == {"multi": 2, "single": 2 * len(ours)}
    assert opt.state[ours[late]]["step"] == 2 and opt.state[ours[0]]["step"] == 4


# ------------------------------------------------------------------------------------------------ weight refresh
CAST_DESC = np.dtype([("w", "<u8"), ("w16", "<u8"), ("wt16", "<u8"), ("N", "<i4"), ("K", "<i4"), ("block0", "<u4"), ("tiles_k", "<u4")])
QUANT_DESC = np.dtype([("w", "<u8"), ("w8", "<u8"), ("w16", "<u8"), ("wt16", "<u8"), ("wt8", "<u8"), ("rexp", "<u8"), ("wtexp", "<u8"),
                       ("N", "<i4"), ("K", "<i4"), ("b0_rows", "<u4"), ("b0_tiles", "<u4"), ("b0_trows", "<u4"), ("tiles_k", "<u4")])


def _to_device_table(rec):
    return torch.from_numpy(rec.view(np.uint8).copy()).to(DEV)


def _ptr(t):
    return 0 if t is None else t.data_ptr()


def _plant_ties(w):
    """every third element becomes an exact bf16 round-to-nearest-even tie (low 16 bits 0x8000: half way between two bf16
    values, with even and odd upper halves alike); row 0 holds the literal 1 + j / 128 + 2^-8 patterns"""
    flat = w.view(-1).view(torch.int32)
    flat[::3] = (flat[::3] & -65536) | 0x8000
    k = w.shape[1]
    w[0] = 1.0 + (torch.arange(k, device=w.device) % 128) / 128.0 + 2.0 ** -8
    return w


# a one-tile tensor (1, 1) between two many-tile ones; (5, 257) is the record without a transposed copy
CAST_SHAPES = ((100, 72), (1, 1), (96, 160), (33, 31), (257, 5), (5, 257), (768, 3), (64, 64))
BF16_GUARD = -7.0


def test_cast_weight_multi_bit_for_bit():
    """clipx_cast_weight_multi against w.to(bfloat16) and its transpose, eight shapes in one launch (single-tile, ragged in N,
    in K, in both, tall and wide), a record with wt16 = NULL, planted round-to-nearest-even ties, one guard row behind every
    output.  The 40-byte records are packed here as include/clipx.h documents them."""
    assert CAST_DESC.itemsize == 40
    rec = np.zeros(len(CAST_SHAPES), dtype=CAST_DESC)
    ws, outs, blk = [], [], 0
    for i, (N, K) in enumerate(CAST_SHAPES):
        gen = torch.Generator().manual_seed(20 + i)
        w = _plant_ties(torch.randn(N, K, generator=gen).to(DEV))
        w16 = torch.full((N + 1, K), BF16_GUARD, dtype=torch.bfloat16, device=DEV)
        wt16 = None if (N, K) == (5, 257) else torch.full((K + 1, N), BF16_GUARD, dtype=torch.bfloat16, device=DEV)
        tk = (K + 31) // 32
        rec[i] = (w.data_ptr(), w16.data_ptr(), _ptr(wt16), N, K, blk, tk)
        blk += ((N + 31) // 32) * tk
        ws.append(w)
        outs.append((w16, wt16))
    originals = [w.clone() for w in ws]
    table = _to_device_table(rec)
    ops.cast_weight_multi(table, len(CAST_SHAPES), blk)
    nulls = 0
    for (N, K), w, w0, (w16, wt16) in zip(CAST_SHAPES, ws, originals, outs):
        assert same_bits(w, w0), (N, K)
        want = w0.to(torch.bfloat16)
        assert bool((want.float() != w0).any()) or (N, K) == (1, 1)       # the inputs do need rounding
        assert same_bits(w16[:N], want), (N, K)
        assert bool((w16[N:] == BF16_GUARD).all()), (N, K)
        if wt16 is None:
            nulls += 1
            continue
        assert same_bits(wt16[:K], want.t().contiguous()), (N, K)
        assert bool((wt16[K:] == BF16_GUARD).all()), (N, K)
    assert nulls == 1


QUANT_SHAPES = ((100, 72), (33, 31), (256, 512), (1280, 264))


def _quant_per_tensor(w):
    N, K = w.shape
    rexp = torch.full((N,), -77, dtype=torch.int32, device=DEV)
    w8 = torch.full((N, K), 0xAB, dtype=torch.uint8, device=DEV)
    w16 = torch.full((N, K), BF16_GUARD, dtype=torch.bfloat16, device=DEV)
    wt16 = torch.full((K, N), BF16_GUARD, dtype=torch.bfloat16, device=DEV)
    ops.quant_weight_e4m3(w, rexp, w8, w16, wt16)
    return rexp, w8, w16, wt16


def _check_quant_against_ref(w, rexp, w8, w16, wt16, label):
    q_ref, e_ref, deq_ref = R.e4m3_rows_ref(w)
    assert torch.equal(rexp, e_ref), label
    assert R.e4m3_bytes_match(w8, q_ref), label
    own = w8.view(torch.float8_e4m3fn).float() * R.pow2(rexp)[:, None]
    assert same_bits(w16, own.to(torch.bfloat16)), label                    # the bf16 copy IS the dequantised byte
    assert torch.equal(w16.float(), deq_ref), label
    assert same_bits(wt16, w16.t().contiguous()), label


@pytest.mark.parametrize("N,K", QUANT_SHAPES)
def test_quant_weight_e4m3_against_reference(N, K):
    """clipx_quant_weight_e4m3: row exponents equal the exact rule (smallest e with amax 2^-e <= 448), bytes equal torch's
    float8_e4m3fn cast of the exactly scaled row, w16 is the dequantised value bit for bit, wt16 its transpose.  Rows scaled
    by 2^(i % 13 - 6), with amax = 448 * 2^j and its fp32 neighbours, a zero row and an outlier row planted."""
    w = R.quant_matrix(N, K, seed=40 + N).to(DEV)
    w0 = w.clone()
    rexp, w8, w16, wt16 = _quant_per_tensor(w)
    assert same_bits(w, w0)
    _check_quant_against_ref(w0, rexp, w8, w16, wt16, (N, K))
    assert len(set(rexp.tolist())) >= 8                                      # the exponents do vary


QMULTI_SHAPES = ((256, 512), (512, 256), (100, 72), (1280, 264))
QMULTI_WITH_T = ((256, 512), (1280, 264))            # (512, 256) could have one (N % 8 == 0) and gets null pointers


@pytest.mark.parametrize("with_trows", [True, False], ids=["trows", "blocks_trows0"])
def test_quant_weight_multi_against_per_tensor_and_reference(with_trows):
    """clipx_quant_weight_multi over four weights in one call (80-byte records as include/clipx.h documents them; wt8 / wtexp
    for two records, null for the other two) against the per-tensor route -- clipx_quant_weight_e4m3, then
    clipx_quant_rows_e4m3 of wt16 -- bit for bit, and against e4m3_rows_ref.  With blocks_trows = 0 the third launch is
    skipped and wt8 / wtexp stay as they were."""
    assert QUANT_DESC.itemsize == 80
    rec = np.zeros(len(QMULTI_SHAPES), dtype=QUANT_DESC)
    ws, outs = [], []
    br = bt = bx = 0
    for i, (N, K) in enumerate(QMULTI_SHAPES):
        w = R.quant_matrix(N, K, seed=60 + i).to(DEV)
        rexp = torch.full((N,), -77, dtype=torch.int32, device=DEV)
        w8 = torch.full((N, K), 0xAB, dtype=torch.uint8, device=DEV)
        w16 = torch.full((N, K), BF16_GUARD, dtype=torch.bfloat16, device=DEV)
        wt16 = torch.full((K, N), BF16_GUARD, dtype=torch.bfloat16, device=DEV)
        has_t = (N, K) in QMULTI_WITH_T
        wt8 = torch.full((K, N), 0xCD, dtype=torch.uint8, device=DEV) if has_t else None
        wtexp = torch.full((K,), -99, dtype=torch.int32, device=DEV) if has_t else None
        tk = (K + 31) // 32
        rec[i] = (w.data_ptr(), w8.data_ptr(), w16.data_ptr(), wt16.data_ptr(), _ptr(wt8), rexp.data_ptr(), _ptr(wtexp),
                  N, K, br, bt, bx, tk)
        br += (N + 3) // 4
        bt += ((N + 31) // 32) * tk
        bx += (K + 3) // 4
        ws.append(w)
        outs.append((rexp, w8, w16, wt16, wt8, wtexp))
    originals = [w.clone() for w in ws]
    table = _to_device_table(rec)
    ops.quant_weight_multi(table, len(QMULTI_SHAPES), br, bt, bx if with_trows else 0)
    for (N, K), w, w0, (rexp, w8, w16, wt16, wt8, wtexp) in zip(QMULTI_SHAPES, ws, originals, outs):
        assert same_bits(w, w0), (N, K)
        rexp1, w81, w161, wt161 = _quant_per_tensor(w0)
        assert torch.equal(rexp, rexp1) and torch.equal(w8, w81) and same_bits(w16, w161) and same_bits(wt16, wt161), (N, K)
        _check_quant_against_ref(w0, rexp, w8, w16, wt16, (N, K))
        if wt8 is None:
            continue
        if not with_trows:
            assert bool((wt8 == 0xCD).all()) and bool((wtexp == -99).all()), (N, K)
            continue
        wt81, wtexp1 = ops.quant_rows_e4m3(wt161)
        assert torch.equal(wtexp, wtexp1) and torch.equal(wt8, wt81), (N, K)
        qt_ref, et_ref, _ = R.e4m3_rows_ref(R.e4m3_rows_ref(w0)[2].t().contiguous())
        assert torch.equal(wtexp, et_ref) and R.e4m3_bytes_match(wt8, qt_ref), (N, K)


@pytest.mark.parametrize("precision", ["fp8", "fp8_mfma"])
def test_fp8_weight_copies_follow_the_optimizer(precision, monkeypatch):
    """The engines' own packers (_refresh_all_quant: the 80-byte table for the block weights, the 40-byte table for the rest) on
    ViT-w256-test, whose block widths meet the fp8 MFMA conditions (K % 128 == 0, K >= 256).  After one FusedAdamW step and one
    more forward every _shadow entry -- w16, wt16, w8, rexp, and wt8 / wtexp where present -- equals the per-tensor
    quantisation of the CURRENT parameter bit for bit, and equals what the same model holds after the per-tensor route
    (CLIPX_QUANT_MULTI=0, read on every forward) refreshed the same weights."""
    import colxlip_amd
    from colxlip_amd import create_model_and_transforms
    from colxlip_amd.data import synthetic_batch
    from colxlip_amd.loss import ClipLoss
    monkeypatch.delenv("CLIPX_QUANT_MULTI", raising=False)
    calls = {"quant": 0, "cast": 0}
    quant_multi, cast_multi = ops.quant_weight_multi, ops.cast_weight_multi

    def counted_quant(*a, **k):
        calls["quant"] += 1
        return quant_multi(*a, **k)

    def counted_cast(*a, **k):
        calls["cast"] += 1
        return cast_multi(*a, **k)
    monkeypatch.setattr(colxlip_amd.ops, "quant_weight_multi", counted_quant)
    monkeypatch.setattr(colxlip_amd.ops, "cast_weight_multi", counted_cast)
    torch.manual_seed(0)
    model, _, _ = create_model_and_transforms("ViT-w256-test", precision=precision, device=DEV, output_dict=True)
    model.train()
    opt = FusedAdamW(param_groups(model.named_parameters(), 0.2), lr=1e-2, betas=R.BETAS, eps=R.EPS)
    images, texts = synthetic_batch(8, model.visual.image_size, model.context_length, model.vocab_size, seed=3, device=DEV,
                                    image_dtype=torch.bfloat16)
    texts = texts[:, 0].contiguous()
    out = model(images, texts)
    ClipLoss()(**out, output_dict=True)["total_loss"].backward()
    before = {k: p.detach().clone() for k, p in model.named_parameters()}
    opt.step()
    assert calls == {"quant": 0, "cast": 0}
    with torch.no_grad():
        model(images, texts)
    assert calls["quant"] == 2                                              # both towers went through the multi-tensor kernels
    params = dict(model.named_parameters())
    snapshot, quantised, with_t, plain_towers = {}, 0, 0, 0
    for prefix, eng in (("visual.", model.visual._engine), ("", model._text_engine)):
        plain_towers += any(not (len(e) >= 6 and e[4] is not None) for e in eng._shadow.values())
        for name, ent in eng._shadow.items():
            if "#" in name:          # `<in_proj_weight>#q` / `#kv`: row ranges of the last block's packed in_proj (split GEMMs)
                base, part = name.split("#")
                full = params[prefix + base].detach()
                p = full[:full.shape[0] // 3] if part == "q" else full[full.shape[0] // 3:]
                moved = True
            else:
                p = params[prefix + name].detach()
                moved = not torch.equal(p, before[prefix + name])
            assert moved, name                                              # the optimizer did change it
            w = (p.view(p.shape[0], -1) if p.ndim != 2 else p).contiguous()
            snapshot[prefix + name] = tuple(t.clone() if torch.is_tensor(t) else t for t in ent)
            if ent[0].shape != w.shape:
                continue
            if len(ent) >= 6 and ent[4] is not None:
                rexp, w8, w16, wt16 = _quant_per_tensor(w)
                assert same_bits(ent[0], w16) and same_bits(ent[1], wt16), name
                assert torch.equal(ent[4], w8) and torch.equal(ent[5], rexp), name
                quantised += 1
                if len(ent) >= 8:
                    wt8, wtexp = ops.quant_rows_e4m3(wt16)
                    assert torch.equal(ent[6], wt8) and torch.equal(ent[7], wtexp), name
                    with_t += 1
            else:
                assert same_bits(ent[0], w.to(torch.bfloat16)), name
                assert same_bits(ent[1], w.t().contiguous().to(torch.bfloat16)), name
    assert calls["cast"] == plain_towers                                    # ... and the plain bf16 copies through theirs
    assert quantised == 2 * 2 * 4                                           # four GEMM weights per block, two blocks per tower
    assert with_t == (quantised if precision == "fp8_mfma" else 0)
    # the same weights through the per-tensor route: every copy made stale again, the multi-tensor kernels switched off
    monkeypatch.setenv("CLIPX_QUANT_MULTI", "0")
    torch.autograd.graph.increment_version(list(model.parameters()))
    done = dict(calls)
    with torch.no_grad():
        model(images, texts)
    assert calls["quant"] == done["quant"]
    compared = 0
    for prefix, eng in (("visual.", model.visual._engine), ("", model._text_engine)):
        for name, ent in eng._shadow.items():
            old = snapshot[prefix + name]
            assert len(ent) == len(old), name
            assert ent[2] != old[2], name                                   # it was refreshed, not kept
            for i in (0, 1) + tuple(range(4, len(ent))):
                assert same_bits(ent[i], old[i]), (name, i)
            compared += 1
    assert compared == len(snapshot)


# ------------------------------------------------------------------------------------------------ flat casts
CAST_BIG = 4 * 256 * 8192 + 4 * 256 + 7                 # more 16-byte groups than the 8192-block grid holds, and a tail
_SPECIAL = [0.0, -0.0, float("inf"), float("-inf"), float("nan"), 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -(2.0 + 2.0 ** -7)]


def _cast_input(n):
    """fp32 values with round-to-nearest-even ties, +-0, +-inf and NaN at the head and in the last elements (the scalar tail)"""
    gen = torch.Generator().manual_seed(n % 1000)
    x = torch.randn(n, generator=gen).to(DEV)
    flat = x.view(torch.int32)
    flat[::3] = (flat[::3] & -65536) | 0x8000
    sp = torch.tensor(_SPECIAL, device=DEV)
    k = min(n, len(_SPECIAL))
    x[:k] = sp.roll(n % len(_SPECIAL))[:k]               # the short sizes each get a different selection
    if n > 2 * len(_SPECIAL):
        x[-len(_SPECIAL):] = sp.flip(0)
    return x


def _same_or_nan(got, want):
    nan = torch.isnan(want)
    return torch.equal(torch.isnan(got), nan) and torch.equal(bits(got)[~nan], bits(want)[~nan])


@pytest.mark.parametrize("scale", [1.0, 0.125])
@pytest.mark.parametrize("n", [1, 3, 4, 5, 1023, CAST_BIG])
def test_flat_casts_bit_for_bit(n, scale):
    """clipx_cast_f32_bf16 against (x * scale).to(bfloat16) and clipx_cast_bf16_f32 against x.float() * scale, bit for bit
    (NaN by isnan), sentinels behind the end."""
    x = _cast_input(n)
    x0 = x.clone()
    y = torch.full((n + 8,), BF16_GUARD, dtype=torch.bfloat16, device=DEV)
    assert ops.cast_f32_bf16(x, y[:n], scale).data_ptr() == y.data_ptr()
    assert _same_or_nan(x, x0)
    assert _same_or_nan(y[:n], (x0 * scale).to(torch.bfloat16))
    assert bool((y[n:] == BF16_GUARD).all())
    if n > 8:
        assert int(torch.isnan(y[:n]).sum()) == 2 and int(torch.isinf(y[:n]).sum()) == 4
    h = y[:n].clone()
    z = torch.full((n + 8,), R.SENTINEL, device=DEV)
    ops.cast_bf16_f32(h, z[:n], scale)
    assert _same_or_nan(h, y[:n])
    assert _same_or_nan(z[:n], h.float() * scale)
    assert bool((z[n:] == R.SENTINEL).all())


@pytest.mark.parametrize("n", [5, 1023])
def test_flat_casts_into_a_slice(n):
    """the bf16 side at an 8-byte-aligned but not 16-byte-aligned offset of a larger buffer (what the alignment contract of
    include/clipx.h allows); the neighbours stay untouched"""
    x = _cast_input(n)
    buf = torch.full((n + 16,), BF16_GUARD, dtype=torch.bfloat16, device=DEV)
    out = buf[4:4 + n]
    assert out.data_ptr() % 16 == 8
    ops.cast_f32_bf16(x, out, 0.125)
    assert _same_or_nan(out, (x * 0.125).to(torch.bfloat16))
    assert bool((buf[:4] == BF16_GUARD).all()) and bool((buf[4 + n:] == BF16_GUARD).all())
    fbuf = torch.full((n + 16,), R.SENTINEL, device=DEV)
    ops.cast_bf16_f32(out, fbuf[4:4 + n], 0.125)                       # source 8-byte aligned, destination 16-byte aligned
    assert _same_or_nan(fbuf[4:4 + n], out.float() * 0.125)
    assert bool((fbuf[:4] == R.SENTINEL).all()) and bool((fbuf[4 + n:] == R.SENTINEL).all())


def test_flat_casts_refuse_what_they_cannot_write():
    """a destination that breaks the documented alignment raises through ops.check and nothing runs; a non-contiguous `out`
    (whose contiguous copy would take the result and be lost) is refused by an assertion"""
    n = 64
    x = torch.randn(n, device=DEV)
    buf = torch.full((n + 8,), BF16_GUARD, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(ClipxError):
        ops.cast_f32_bf16(x, buf[1:1 + n])                                # 2-byte aligned destination
    with pytest.raises(ClipxError):
        ops.cast_f32_bf16(torch.randn(n + 1, device=DEV)[1:], buf[:n])    # 4-byte aligned source
    assert bool((buf == BF16_GUARD).all())
    fbuf = torch.full((n + 8,), R.SENTINEL, device=DEV)
    h = torch.ones(n + 8, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(ClipxError):
        ops.cast_bf16_f32(h[:n], fbuf[1:1 + n])                           # 4-byte aligned destination
    with pytest.raises(ClipxError):
        ops.cast_bf16_f32(h[1:1 + n], fbuf[:n])                           # 2-byte aligned source
    assert bool((fbuf == R.SENTINEL).all())
    strided16 = torch.full((2 * n,), BF16_GUARD, dtype=torch.bfloat16, device=DEV)[::2]
    strided32 = torch.full((2 * n,), R.SENTINEL, device=DEV)[::2]
    with pytest.raises(AssertionError):
        ops.cast_f32_bf16(x, strided16)
    with pytest.raises(AssertionError):
        ops.cast_bf16_f32(h[:n], strided32)
    assert bool((strided16 == BF16_GUARD).all()) and bool((strided32 == R.SENTINEL).all())


# ------------------------------------------------------------------------------------------------ sumsq, scale
def _sumsq_additions(n):
    """How many fp32 roundings a term x_i^2 can pass through in sumsq_kernel, read off the kernel: the square itself (1); the
    thread's serial sum over its grid-stride elements, ceil(n / (blocks * 256)) of them; the wave's butterfly, log2(64) = 6;
    the four wave partials, (a + b) + (c + d), 2; and one atomicAdd per block onto the single accumulator, which in the worst
    order carries a term (and the initial value) through all `blocks` of them."""
    blocks = min((n + 1023) // 1024, 2048)
    return 1 + -(-n // (blocks * 256)) + 6 + 2 + blocks


@pytest.mark.parametrize("n", [1, 1025, 2048 * 1024 + 77])
def test_sumsq_accumulates_within_its_rounding_bound(n):
    """clipx_sumsq onto a NON-zero accumulator against the fp64 sum.  Every term is non-negative, so the relative error is at
    most c 2^-24 / (1 - c 2^-24) with c the number of roundings a term can pass through (_sumsq_additions): 2062 at the
    largest size, past the 2048-block grid cap -- a bound of 1.23e-4, where a dropped block or a dropped tail is off by 5e-4
    and more."""
    c = _sumsq_additions(n)
    assert c == {1: 11, 1025: 14, 2048 * 1024 + 77: 2062}[n]
    gen = torch.Generator().manual_seed(n % 97)
    x = torch.randn(n, generator=gen).to(DEV)
    x[-1] = 40.0                                         # the last element (the grid-stride tail) carries weight
    start = 3.25
    acc = torch.tensor([start], device=DEV)
    ops.sumsq(x, acc)
    want = start + float((x.double() ** 2).sum())
    bound = c * R.U32 / (1 - c * R.U32)
    err = abs(float(acc) - want) / want
    print(f"[sumsq] n {n}: rel err {err:.3e}  bound {bound:.3e}")
    assert err <= bound, (n, err, bound)
    assert 1600.0 / want > 4 * bound                     # ... so that dropping it would be seen


SCALE_N = 4096 * 256 + 256 + 3                          # past the 4096-block caps of both scale kernels


def test_scale_kernels_bit_for_bit():
    """clipx_scale (in place) and clipx_scale_by_dev (out of place and in place, out = x) against x * s, past their grid caps"""
    gen = torch.Generator().manual_seed(9)
    x0 = torch.randn(SCALE_N, generator=gen).to(DEV)
    s = 0.37
    want = x0 * torch.tensor(s, dtype=torch.float32, device=DEV)
    assert bool((want != x0).all())
    buf = torch.full((SCALE_N + 4,), R.SENTINEL, device=DEV)
    buf[:SCALE_N] = x0
    ops.scale_(buf[:SCALE_N], s)
    assert same_bits(buf[:SCALE_N], want) and bool((buf[SCALE_N:] == R.SENTINEL).all())
    s_dev = torch.tensor([s], device=DEV)
    x = x0.clone()
    out = ops.scale_by_dev(x, s_dev)
    assert same_bits(out, want) and same_bits(x, x0)
    buf[:SCALE_N] = x0
    assert ops.scale_by_dev(buf[:SCALE_N], s_dev, out=buf[:SCALE_N]).data_ptr() == buf.data_ptr()
    assert same_bits(buf[:SCALE_N], want) and bool((buf[SCALE_N:] == R.SENTINEL).all())
    assert float(s_dev) == R.f32(s)
