"""The references of tests/update_path_ref.py checked on the CPU, and the AdamW tolerance of the kernel tests fixed here:
adamw_ref is torch.optim.AdamW, e4m3_row_exp is the brute-force exponent, and the fp32 emulation of the kernel's formula
lies within one eighth of the constants the GPU tests allow."""
import pytest
import torch

from tests import update_path_ref as R


@pytest.mark.parametrize("wd", [0.0, 0.2])
@pytest.mark.parametrize("gscale", [1.0, 0.37])
def test_adamw_ref_is_torch_adamw(wd, gscale):
    """Five steps of torch.optim.AdamW on fp64 CPU tensors against adamw_ref fed with its own output.  torch works on the
    Python doubles, adamw_ref on the hyper-parameters rounded to fp32 (what the kernel gets).  The largest such difference is
    1 - 0.98f against 0.02: 2^-24 * 0.98 / 0.02 = 49 * 2^-24 relative on one term of v' (9 * 2^-24 for 1 - 0.9f, 1 * 2^-24 for
    lr, eps and the bias corrections).  m' and v' are convex combinations, so their error stays at that size from step to
    step; p' adds one update's error per step.  Hence 64 * 2^-24 * step, relative to the magnitude sums; a wrong formula is
    off by orders of magnitude more."""
    n, lr = 2000, 5e-4
    p0, _, _, _ = R.adamw_values(n, 1)
    ref_p = torch.nn.Parameter(p0.double())
    opt = torch.optim.AdamW([ref_p], lr=lr, betas=R.BETAS, eps=R.EPS, weight_decay=wd)
    p, m, v = p0.double(), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    for step in range(1, 6):
        g = R.adamw_values(n, 10 + step)[1].double()
        ref_p.grad = g * gscale                      # the kernel's gscale is a pre-multiplied gradient
        opt.step()
        p, m, v, (sp, sm, sv) = R.adamw_ref(p, g, m, v, lr, *R.BETAS, R.EPS, wd, step, gscale)
        st = opt.state[ref_p]
        for got, want, scale in ((p, ref_p.detach(), sp), (m, st["exp_avg"], sm), (v, st["exp_avg_sq"], sv)):
            assert float(((got - want).abs() / scale).max()) < 64 * R.U32 * step, step
        assert float((p - p0.double()).abs().max()) > 0.5 * lr          # it did move


def test_adamw_ref_takes_a_weight_decay_per_element():
    p, g, m, v = R.adamw_values(64, 2)
    wd = torch.tensor([0.0, 0.2] * 32)
    both = R.adamw_ref(p, g, m, v, 5e-4, *R.BETAS, R.EPS, wd, 3, 0.37)
    for k, w in ((0, 0.0), (1, 0.2)):
        one = R.adamw_ref(p[k::2], g[k::2], m[k::2], v[k::2], 5e-4, *R.BETAS, R.EPS, w, 3, 0.37)
        assert torch.equal(both[0][k::2], one[0]) and torch.equal(both[3][0][k::2], one[3][0])


def test_adamw_layouts():
    """what the kernel tests rely on: alignment classes, guard elements between neighbours, sizes and counts"""
    layout, total = R.mixed_layout()
    assert len(layout) == 27 and sorted({n for n, _, _ in layout}) == sorted(R.MIXED_SIZES)
    assert [tuple(o % 4 for o in offs) for _, offs, _ in layout] == list(R.MIXED_SHIFTS) * 9
    assert [wd for _, _, wd in layout] == [0.0, 0.2] * 13 + [0.0]
    many, mtotal = R.many_layout()
    assert len(many) == 301 and sum(n for n, _, _ in many) < 1_000_000
    assert min(n for n, _, _ in many) == 1 and max(n for n, _, _ in many) > 4096 and all(1 <= n <= 5000 for n, _, _ in many)
    assert len({wd for _, _, wd in many}) == 301
    for lay, tot in ((layout, total), (many, mtotal)):
        for s in range(4):
            spans = sorted((offs[s], offs[s] + n) for n, offs, _ in lay)
            assert spans[0][0] >= 1 and spans[-1][1] < tot
            assert all(b[0] - a[1] >= 1 for a, b in zip(spans, spans[1:]))
            assert int(R.guard_mask(lay, tot, s).sum()) == tot - sum(n for n, _, _ in lay)
    assert R.CAP_N // 4 > 4096 * 256 and R.CAP_N % 4 == 3


def test_adamw_tolerance_constants():
    """The op-by-op fp32 emulation of the kernel's formula, on exactly the inputs of the kernel tests, against adamw_ref: its
    largest deviation in units of 2^-24 * magnitude sum must lie within the recorded ADAMW_EMU_DEV_*, i.e. one eighth of what
    the kernel tests allow -- a change of the inputs cannot silently outgrow the constants."""
    worst = [0.0, 0.0, 0.0]
    for name, p, g, m, v, wd, lr, step, gs in R.adamw_cases():
        ref = R.adamw_ref(p, g, m, v, lr, *R.BETAS, R.EPS, wd, step, gs)
        emu = R.adamw_emulate_f32(p, g, m, v, lr, *R.BETAS, R.EPS, wd, step, gs)
        dev = R.adamw_deviation(emu, ref)
        print(f"[adamw emulation] {name}: n {p.numel()}  dev p {dev[0]:.3f}  m {dev[1]:.3f}  v {dev[2]:.3f}  (x 2^-24 x magnitude)")
        worst = [max(a, b) for a, b in zip(worst, dev)]
    print(f"[adamw emulation] worst: p {worst[0]:.3f}  m {worst[1]:.3f}  v {worst[2]:.3f}")
    assert worst[0] <= R.ADAMW_EMU_DEV_P and worst[1] <= R.ADAMW_EMU_DEV_M and worst[2] <= R.ADAMW_EMU_DEV_V, worst
    assert (R.ADAMW_TOL_P, R.ADAMW_TOL_M, R.ADAMW_TOL_V) == (8 * R.ADAMW_EMU_DEV_P, 8 * R.ADAMW_EMU_DEV_M, 8 * R.ADAMW_EMU_DEV_V)
    # the constants are a measurement, not head-room: the emulation reaches at least half of each
    assert all(w >= 0.5 * c for w, c in zip(worst, (R.ADAMW_EMU_DEV_P, R.ADAMW_EMU_DEV_M, R.ADAMW_EMU_DEV_V))), worst


def _brute_exp(amax: float) -> int:
    """smallest e in [-200, 200] with amax * 2^-e <= 448, by search in exact arithmetic (Python floats scale by powers of
    two without rounding in this range)"""
    if amax == 0.0:
        return 0
    return next(e for e in range(-200, 201) if amax * 2.0 ** -e <= 448.0)


def test_e4m3_row_exponent_rule():
    K = 40
    rows = R.planted_rows(K)
    assert rows.shape[0] == 3 * len(R.PLANT_J) + 2
    amax = rows.abs().amax(1)
    for i, j in enumerate(R.PLANT_J):                 # the rows really sit below, on and above 448 * 2^j
        below, on, above = (float(a) for a in amax[3 * i:3 * i + 3])
        assert below < on == 448.0 * 2.0 ** j < above
        assert [_brute_exp(a) for a in (below, on, above)] == [j, j, j + 1]
    assert float(amax[-2]) == 0.0 and float(amax[-1]) == 3.0 * 2.0 ** 20
    generic = torch.randn(64, K) * R.pow2(torch.arange(64) % 13 - 6)[:, None]
    for w in (rows, generic, generic.bfloat16()):
        e = R.e4m3_row_exp(w)
        assert e.dtype == torch.int32
        assert e.tolist() == [_brute_exp(float(a)) for a in w.float().abs().amax(1)]


def test_e4m3_rows_ref_bytes_and_dequantisation():
    w = R.quant_matrix(100, 72, seed=3)
    q, e, deq = R.e4m3_rows_ref(w)
    assert q.dtype == torch.uint8 and q.shape == w.shape and deq.dtype == torch.float32
    scaled = w.double() * (2.0 ** -e.double())[:, None]
    assert float(scaled.abs().max()) <= 448.0                            # no saturation ...
    nzrow = w.abs().amax(1) > 0
    assert float(scaled.abs().amax(1)[nzrow].min()) > 224.0                # ... and no wasted bit
    val = q.view(torch.float8_e4m3fn).double()
    assert torch.equal(deq.double(), val * (2.0 ** e.double())[:, None])
    # round to nearest: within half a step of the e4m3 grid (step 2^(floor(log2 |x|) - 3), 2^-9 in the subnormal range)
    step = torch.exp2(torch.floor(torch.log2(scaled.abs().clamp_min(2.0 ** -6))) - 3)
    assert bool(((val - scaled).abs() <= step / 2).all())
    assert torch.equal(deq.bfloat16().float(), deq)                        # exact in bf16
    assert R.e4m3_bytes_match(q, q) and not R.e4m3_bytes_match(q ^ 1, q)
    assert torch.equal(R.pow2(torch.arange(-126, 128)).double(), 2.0 ** torch.arange(-126, 128).double())
