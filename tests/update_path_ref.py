"""Test helper: plain references for the kernels that end every training step (csrc/elementwise.hip: clipx_adamw[_multi],
clipx_quant_weight_e4m3 / _multi), the inputs the AdamW tests run on, and the tolerance those tests allow.  torch only, on
the CPU or on the tensors' device.  It lives with the tests because the product has no CPU path."""
import torch

U32 = 2.0 ** -24            # unit roundoff of fp32 (round to nearest)

# ---- AdamW tolerance --------------------------------------------------------------------------------------------------
# |kernel - adamw_ref| <= ADAMW_TOL_x * 2^-24 * (magnitude sum of the quantity, see adamw_ref), element by element.
# Origin: adamw_emulate_f32 below restates the kernel's formula op by op in fp32 without FMA; over every input set of
# adamw_cases() its largest deviation from adamw_ref, in those units, is ADAMW_EMU_DEV_x (measured on the CPU by
# tests/test_update_path_cpu.py, which asserts that the emulation still lies within them).  The kernel tests allow 8 times
# that: FMA contraction and a differently rounded sqrt or divide change individual roundings, not how many there are.
# Never tuned to what the HIP kernel returns.
ADAMW_EMU_DEV_P = 9.11         # measured 9.105 (the 301-tensor launch: m' cancels, which the scale |update| does not see)
ADAMW_EMU_DEV_M = 2.55         # measured 2.544
ADAMW_EMU_DEV_V = 3.89         # measured 3.888
ADAMW_TOL_P = 8 * ADAMW_EMU_DEV_P
ADAMW_TOL_M = 8 * ADAMW_EMU_DEV_M
ADAMW_TOL_V = 8 * ADAMW_EMU_DEV_V

ADAMW_BLOCK = 4096          # ADAMW_BLOCK_ELEMS in csrc/elementwise.hip
SENTINEL = -12345.625       # guard elements between the tensors of an arena
BETAS = (0.9, 0.98)
EPS = 1e-6


def f32(x) -> float:
    """a Python number as the kernel receives it: rounded to float"""
    return float(torch.tensor(float(x), dtype=torch.float32))


def adamw_hyper(lr, b1, b2, eps, step, gscale):
    """The fp32 scalars a launch gets, as doubles.  bc1 / bc2 are computed in Python doubles from the unrounded betas and
    then passed as float, exactly as ops.adamw / ops.adamw_multi do."""
    return dict(lr=f32(lr), b1=f32(b1), b2=f32(b2), eps=f32(eps), gscale=f32(gscale),
                bc1=f32(1.0 - b1 ** step), bc2=f32(1.0 - b2 ** step))


def _wd64(wd, like):
    """weight decay (a number, or one value per element) rounded to fp32, as fp64 on `like`'s device"""
    if torch.is_tensor(wd):
        return wd.to(device=like.device, dtype=torch.float32).double()
    return torch.tensor(f32(wd), dtype=torch.float64, device=like.device)


def adamw_ref(p, g, m, v, lr, b1, b2, eps, wd, step, gscale=1.0):
    """One AdamW step in fp64, the formula of include/clipx.h on the fp32-rounded hyper-parameters:
    g *= gscale; m' = b1 m + (1-b1) g; v' = b2 v + (1-b2) g^2; p' = p (1 - lr wd) - (lr / bc1) m' / (sqrt(v') / sqrt(bc2) + eps).
    wd is a number or a tensor with one value per element.  Returns (p', m', v', (sp, sm, sv)): the magnitude sums
    sp = |p (1 - lr wd)| + |update|, sm = |b1 m| + |(1-b1) g|, sv = |b2 v| + |(1-b2) g^2| that an error bound is scaled by
    (m' can cancel, so |m'| is no scale)."""
    h = adamw_hyper(lr, b1, b2, eps, step, gscale)
    p, g, m, v = (t.double() for t in (p, g, m, v))
    wd = _wd64(wd, p)
    g = g * h["gscale"]
    m_a, m_b = h["b1"] * m, (1.0 - h["b1"]) * g
    v_a, v_b = h["b2"] * v, (1.0 - h["b2"]) * g * g
    m1, v1 = m_a + m_b, v_a + v_b
    upd = (h["lr"] / h["bc1"]) * m1 / (v1.sqrt() / (h["bc2"] ** 0.5) + h["eps"])
    p_a = p * (1.0 - h["lr"] * wd)
    return p_a - upd, m1, v1, (p_a.abs() + upd.abs(), m_a.abs() + m_b.abs(), v_a.abs() + v_b.abs())


def adamw_emulate_f32(p, g, m, v, lr, b1, b2, eps, wd, step, gscale=1.0):
    """adamw_multi_kernel / adamw_kernel restated op by op on fp32 tensors: every product, sum, sqrt and quotient is its own
    torch op and so rounded on its own (no FMA), the scalars are formed in fp32 the way the kernel and its launcher form them."""
    h = adamw_hyper(lr, b1, b2, eps, step, gscale)
    t = lambda x: torch.tensor(x, dtype=torch.float32)          # noqa: E731
    one = t(1.0)
    lr_, b1_, b2_, eps_, gs = t(h["lr"]), t(h["b1"]), t(h["b2"]), t(h["eps"]), t(h["gscale"])
    inv_bc1 = one / t(h["bc1"])
    inv_sqrt_bc2 = one / t(h["bc2"]).sqrt()
    wd_ = wd.float() if torch.is_tensor(wd) else t(f32(wd))
    decay = one - lr_ * wd_
    stp = lr_ * inv_bc1
    gr = g * gs
    m1 = b1_ * m + (one - b1_) * gr
    v1 = b2_ * v + ((one - b2_) * gr) * gr
    p1 = p * decay - stp * (m1 / (v1.sqrt() * inv_sqrt_bc2 + eps_))
    return p1, m1, v1


def adamw_deviation(got, ref):
    """largest |got - ref| of p, m, v in units of 2^-24 * magnitude sum; (dp, dm, dv) as floats"""
    out = []
    for x, r, s in zip(got, ref[:3], ref[3]):
        out.append(float(((x.double() - r).abs() / (U32 * s)).max()))
    return tuple(out)


def adamw_within(got, ref):
    """per-element verdicts: (p ok, m ok, v ok) boolean tensors under ADAMW_TOL_*"""
    return tuple((x.double() - r).abs() <= tol * U32 * s
                 for x, r, s, tol in zip(got, ref[:3], ref[3], (ADAMW_TOL_P, ADAMW_TOL_M, ADAMW_TOL_V)))


# ---- AdamW inputs (the CPU test measures the tolerance on exactly what the kernel tests launch) ----------------------
def adamw_values(n, seed):
    """(p, g, m, v) flat fp32 CPU tensors: g over four decades, m and v non-zero, v > 0"""
    gen = torch.Generator().manual_seed(seed)
    p = torch.randn(n, generator=gen)
    g = torch.randn(n, generator=gen) * torch.pow(10.0, torch.rand(n, generator=gen) * 4.0 - 3.0)
    m = torch.randn(n, generator=gen) * 0.1
    v = torch.rand(n, generator=gen) * 1e-2 + 1e-6
    return p, g, m, v


MIXED_SIZES = (1, 3, 255, 4095, 4096, 4097, 2 * 4096, 2 * 4096 + 5, 3 * 4096 + 1023)
# element offsets of (p, g, m, v) from a 16-byte boundary: all aligned; only p off by one; only v off by two
MIXED_SHIFTS = ((0, 0, 0, 0), (1, 0, 0, 0), (0, 0, 0, 2))


def mixed_layout():
    """[(n, (p, g, m, v element offsets), wd)] of the mixed launch and the arenas' length.  Every tensor starts at a 16-byte
    boundary plus its stream's shift, at least one guard element lies between neighbours, wd alternates 0 / 0.2."""
    out, cur = [], 4
    for n in MIXED_SIZES:
        for shift in MIXED_SHIFTS:
            out.append((n, tuple(cur + s for s in shift), 0.2 if len(out) % 2 else 0.0))
            cur = (cur + 2 + n + 1 + 3) // 4 * 4
    return out, cur + 4


def many_layout(count=301):
    """301 small tensors, sizes cycling through 1..5000 (under 1 M elements in all), tensor i with weight decay 0.001 i; every
    third one starts one element off the 16-byte grid in all four streams."""
    out, cur = [], 4
    for i in range(count):
        n = 1 + (i * 1237) % 5000
        off = cur + (1 if i % 3 == 2 else 0)
        out.append((n, (off, off, off, off), 0.001 * i))
        cur = (cur + 1 + n + 1 + 3) // 4 * 4
    return out, cur + 4


def fill_arenas(layout, total, seed):
    """four flat fp32 CPU arenas [p, g, m, v] with adamw_values in the tensors' slots and SENTINEL everywhere else"""
    vals = adamw_values(sum(n for n, _, _ in layout), seed)
    arenas = [torch.full((total,), SENTINEL, dtype=torch.float32) for _ in range(4)]
    src = 0
    for n, offs, _ in layout:
        for a, x, o in zip(arenas, vals, offs):
            a[o:o + n] = x[src:src + n]
        src += n
    return arenas


def arena_views(arenas, layout):
    """[(p, g, m, v, wd)] views into the arenas, the entries FusedAdamW._multi_table packs"""
    return [tuple(a[o:o + n] for a, o in zip(arenas, offs)) + (wd,) for n, offs, wd in layout]


def guard_mask(layout, total, stream):
    mask = torch.ones(total, dtype=torch.bool)
    for n, offs, _ in layout:
        mask[offs[stream]:offs[stream] + n] = False
    return mask


SINGLE_N = 5000                                  # ntensors = 1: one full block and a tail
CAP_N = 4 * 256 * 4096 + 4 * 256 + 3             # clipx_adamw past its 4096-block grid cap, with an n & 3 tail

# (name, lr, step, gscale) of every launch of the kernel tests
MIXED_RUNS = tuple((f"mixed-step{s}-gscale{gs}", 5e-4, s, gs) for s in (1, 1000) for gs in (1.0, 0.37))
MANY_RUN = ("many", 1e-2, 7, 1.0)
SINGLE_RUN = ("single", 5e-4, 3, 0.37)
CAP_RUN = ("cap", 5e-4, 2, 0.37)
CAP_WD = 0.2
SINGLE_WD = 0.2


def mixed_arenas():
    layout, total = mixed_layout()
    return layout, total, fill_arenas(layout, total, 11)


def many_arenas():
    layout, total = many_layout()
    return layout, total, fill_arenas(layout, total, 12)


def single_values():
    return adamw_values(SINGLE_N, 13)


def cap_values():
    return adamw_values(CAP_N, 14)


def gather(arenas, layout):
    """the tensors of a layout, stream by stream, as four flat vectors [p, g, m, v] (guards left out)"""
    return [torch.cat([arenas[s][offs[s]:offs[s] + n] for n, offs, _ in layout]) for s in range(4)]


def wd_vector(layout):
    return torch.cat([torch.full((n,), wd, dtype=torch.float32) for n, _, wd in layout])


def adamw_cases():
    """Every input set the AdamW kernel tests launch: yields (name, p, g, m, v, wd per element, lr, step, gscale), flat, on
    the CPU."""
    layout, _, arenas = mixed_arenas()
    for name, lr, step, gs in MIXED_RUNS:
        yield (name, *gather(arenas, layout), wd_vector(layout), lr, step, gs)
    layout, _, arenas = many_arenas()
    name, lr, step, gs = MANY_RUN
    yield (name, *gather(arenas, layout), wd_vector(layout), lr, step, gs)
    name, lr, step, gs = SINGLE_RUN
    yield (name, *single_values(), torch.full((SINGLE_N,), SINGLE_WD), lr, step, gs)
    name, lr, step, gs = CAP_RUN
    yield (name, *cap_values(), torch.full((CAP_N,), CAP_WD), lr, step, gs)


# ---- e4m3 weight rows -------------------------------------------------------------------------------------------------
def pow2(e):
    """2^e for an integer tensor, exactly, by building the fp32 exponent field (e in the normal range)"""
    e = e.to(torch.int32)
    assert int(e.min()) >= -126 and int(e.max()) <= 127
    return ((e + 127) << 23).view(torch.float32)


def e4m3_row_exp(w):
    """per row of a 2-D fp32 / bf16 matrix: the smallest e with amax * 2^-e <= 448, 0 for an all-zero row.  Exact:
    amax = fr * 2^ex with fr in [0.5, 1) from torch.frexp, and 448 = 0.875 * 2^9."""
    amax = w.float().abs().amax(1)
    fr, ex = torch.frexp(amax)
    e = torch.where(fr <= 0.875, ex - 9, ex - 8).to(torch.int32)
    return torch.where(amax > 0, e, torch.zeros_like(e))


def e4m3_rows_ref(w):
    """(bytes [N,K] uint8, row_exp [N] int32, dequantised [N,K] fp32) of the row-wise e4m3 quantisation: the bytes are
    torch.float8_e4m3fn of the exactly scaled row, the dequantised values byte * 2^e."""
    e = e4m3_row_exp(w)
    q = (w.float() * pow2(-e)[:, None]).to(torch.float8_e4m3fn)
    return q.view(torch.uint8), e, q.float() * pow2(e)[:, None]


def e4m3_bytes_match(got, ref):
    """magnitude bits everywhere, the sign only where the magnitude is non-zero (a rounded-away value may keep its sign)"""
    nz = (ref & 0x7f) != 0
    return torch.equal(got & 0x7f, ref & 0x7f) and torch.equal((got >> 7)[nz], (ref >> 7)[nz])


PLANT_J = (-9, -1, 0, 3, 8)


def planted_rows(K, seed=5):
    """[R, K] fp32 rows on which the exponent rule can go wrong: amax exactly 448 * 2^j and its fp32 neighbours below and above
    for several j, a zero row, a row whose one outlier is 2^20 times the rest.  K >= 2."""
    gen = torch.Generator().manual_seed(seed)
    rows = []
    for j in PLANT_J:
        top = torch.tensor(448.0 * 2.0 ** j, dtype=torch.float32)
        for amax in (torch.nextafter(top, torch.tensor(0.0)), top, torch.nextafter(top, torch.tensor(float("inf")))):
            r = (torch.rand(K, generator=gen) * 2 - 1) * amax * 0.99
            r[int(torch.randint(K, (1,), generator=gen))] = amax * (1.0 if len(rows) % 2 else -1.0)
            rows.append(r)
    rows.append(torch.zeros(K))
    r = torch.randn(K, generator=gen).clamp(-3, 3)
    r[K // 2] = 3.0 * 2.0 ** 20
    rows.append(r)
    return torch.stack(rows)


def quant_matrix(N, K, seed):
    """[N, K] fp32 weight for the quantiser tests: row i scaled by 2^(i % 13 - 6), the planted rows spread over it"""
    gen = torch.Generator().manual_seed(seed)
    w = torch.randn(N, K, generator=gen) * 0.05 * pow2(torch.arange(N) % 13 - 6)[:, None]
    plant = planted_rows(K, seed=seed + 1)
    idx = torch.linspace(0, N - 1, plant.shape[0]).long()
    assert idx.unique().numel() == plant.shape[0]
    w[idx] = plant
    return w
