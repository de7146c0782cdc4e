"""Per-kernel parity: each HIP entry point (through the C ABI) against a plain PyTorch fp32
reference of the same op, on seeded inputs.  fp32 mode: tight tolerances (exact-f32 MFMA);
bf16 mode: error measured relative to the fp32 result's scale, bound stated per test."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from colxlip_amd import ops  # noqa: E402
from colxlip_amd._lib import ACT_GELU, ACT_NONE, ACT_QUICKGELU  # noqa: E402

DEV = "cuda"


def rnd(*shape, seed=0, scale=1.0, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(DEV).to(dtype)


def relerr(a, b):
    a, b = a.float(), b.float()
    a, b = a.detach(), b.detach()
    return float((a - b).abs().max() / (b.abs().max() + 1e-12))


def tol(dtype):
    return 2e-5 if dtype == torch.float32 else 2e-2


def act_ref(kind, x):
    if kind == ACT_GELU:
        return torch.nn.functional.gelu(x)
    if kind == ACT_QUICKGELU:
        return x * torch.sigmoid(1.702 * x)
    return x


def act_grad_ref(kind, x):
    x = x.detach().clone().requires_grad_(True)
    act_ref(kind, x).sum().backward()
    return x.grad


# ------------------------------------------------------------------ GEMMs
@pytest.mark.parametrize("M,N,K", [(64, 64, 64), (100, 72, 40), (257, 130, 520), (1, 512, 768), (50, 8, 8)])
def test_gemm_f32_strided(M, N, K):
    A = rnd(M, K, seed=1)
    B = rnd(K, N, seed=2)
    C0 = rnd(M, N, seed=3)
    ref = 0.5 * A @ B + 2.0 * C0
    C = C0.clone()
    ops.gemm_f32(M, N, K, A, K, 1, B, N, 1, C, N, 0.5, 2.0)
    assert relerr(C, ref) < 1e-5
    # transposed operands through strides
    At, Bt = A.t().contiguous(), B.t().contiguous()
    C = torch.empty(M, N, device=DEV)
    ops.gemm_f32(M, N, K, At, 1, M, Bt, 1, K, C, N)
    assert relerr(C, A @ B) < 1e-5


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("M,N,K", [(128, 128, 64), (200, 192, 64), (77, 256, 128), (1000, 768, 512), (40, 64, 64), (392, 64, 768)])
@pytest.mark.parametrize("act", [ACT_NONE, ACT_GELU, ACT_QUICKGELU])
def test_linear_fwd(dtype, M, N, K, act):
    x = rnd(M, K, seed=1, dtype=dtype)
    w = rnd(N, K, seed=2, scale=K ** -0.5, dtype=dtype)
    bias = rnd(N, seed=3)
    res = rnd(M, N, seed=4, dtype=dtype)
    y, u = ops.linear_fwd(x, w, bias, act=act, want_preact=True, residual=res)
    u_ref = x.float() @ w.float().t() + bias
    y_ref = act_ref(act, u_ref) + res.float()
    assert relerr(u, u_ref) < tol(dtype)
    assert relerr(y, y_ref) < tol(dtype)
    y2 = ops.linear_fwd(x, w, None, out_dtype=torch.float32)
    assert y2.dtype == torch.float32
    assert relerr(y2, x.float() @ w.float().t()) < (1e-5 if dtype == torch.float32 else 1e-2)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("M,N,K", [(128, 128, 128), (200, 256, 64), (77, 64, 256), (1000, 512, 768)])
def test_linear_dgrad(dtype, M, N, K):
    dy = rnd(M, N, seed=1, dtype=dtype)
    w = rnd(N, K, seed=2, scale=N ** -0.5, dtype=dtype)
    wt = w.t().contiguous()
    u = rnd(M, K, seed=3, dtype=dtype)
    ref = dy.float() @ w.float()
    if dtype == torch.float32:
        dx = ops.linear_dgrad(dy, w, None)
    else:
        dx = ops.linear_dgrad(dy, None, wt)
    assert relerr(dx, ref) < tol(dtype)
    for act in (ACT_GELU, ACT_QUICKGELU):
        uf = u.float().detach().clone().requires_grad_(True)
        act_ref(act, uf).backward(ref)
        buf = u.clone()
        dx = ops.linear_dgrad(dy, w if dtype == torch.float32 else None, None if dtype == torch.float32 else wt,
                              act=act, u=buf, out=buf)   # in place over u
        assert relerr(dx, uf.grad) < tol(dtype)


@pytest.mark.parametrize("M,N,K", [(512, 768, 3072), (300, 128, 512), (256, 256, 256)])
def test_linear_bf16_epilogue_operands(M, N, K):
    """Full 256x256 / 128x256 tiles take the widened epilogue (16-B operand loads, un-swapped): GELU' multiply,
    residual add and the pre-activation store against the plain formulas."""
    dt = torch.bfloat16
    dy = rnd(M, N, seed=1, dtype=dt)
    wt = rnd(K, N, seed=2, scale=N ** -0.5, dtype=dt)
    u = rnd(M, K, seed=3, dtype=dt)
    ref = dy.float() @ wt.float().t()
    for act in (ACT_GELU, ACT_QUICKGELU):
        uf = u.float().detach().clone().requires_grad_(True)
        act_ref(act, uf).backward(ref)
        dx = ops.linear_dgrad(dy, None, wt, act=act, u=u)
        assert relerr(dx, uf.grad) < tol(dt)
    res = rnd(M, K, seed=4, dtype=dt)
    bias = rnd(K, seed=5)
    y, pre = ops.linear_fwd(dy, wt, bias, act=ACT_GELU, want_preact=True, residual=res)
    assert relerr(pre, ref + bias) < tol(dt)
    assert relerr(y, act_ref(ACT_GELU, ref + bias) + res.float()) < tol(dt)


def test_linear_bf16_beyond_2_31_elements():
    """ViT-L/14-336 at per-GPU batch 1024: M = 590848 rows, N = 4096 -> M*N > 2^31 elements.  Forward (bias + GELU +
    pre-activation, through the pipelined kernel), dgrad x GELU'(u) and wgrad against torch on row slices from the start, the
    middle and the end: every index computation must be 64-bit."""
    M, N, K = 590848, 4096, 1024
    dt = torch.bfloat16
    x = rnd(M, K, seed=1, dtype=dt)
    w = rnd(N, K, seed=2, scale=K ** -0.5, dtype=dt)
    b = rnd(N, seed=3)
    y, u = ops.linear_fwd(x, w, b, act=ACT_GELU, want_preact=True)
    dy = rnd(M, K, seed=4, dtype=dt)
    dx = ops.linear_dgrad(dy, None, w, act=ACT_GELU, u=u)
    for r0 in (0, M // 2 - 128, M - 256):
        sl = slice(r0, r0 + 256)
        ref_u = x[sl].float() @ w.float().t() + b
        assert relerr(u[sl], ref_u) < 2e-2 and relerr(y[sl], act_ref(ACT_GELU, ref_u)) < 2e-2
        uf = u[sl].float().requires_grad_(True)
        act_ref(ACT_GELU, uf).backward(dy[sl].float() @ w.float().t())
        assert relerr(dx[sl], uf.grad) < 2e-2
    del dx, y
    dw = torch.empty(N, K, device=DEV)
    ws = torch.empty(ops.linear_wgrad_ws_bytes(dt, M, N, K), dtype=torch.uint8, device=DEV)
    ops.linear_wgrad(u, x, dw, 0.0, ws)
    ref = torch.zeros(256, K, device=DEV)
    for r0 in range(0, M, 65536):
        ref += u[r0:r0 + 65536, -256:].float().t() @ x[r0:r0 + 65536].float()
    assert relerr(dw[-256:], ref) < 1e-2


@pytest.mark.parametrize("K", [512, 768, 1024, 64])
def test_linear_bf16_pipelined_kernel(K):
    """The opt-in one-wave-per-SIMD NT kernel (deferred, wave-transposed epilogue) against the default kernel and the
    fp32 formulas, on a problem large enough to take 256x256 tiles: K = 512 / 768 park two tuples per k-step, 1024 one,
    64 is too short to defer (falls back to the default kernel)."""
    from colxlip_amd import _lib
    lib = _lib.lib()
    dt = torch.bfloat16
    M, N = 33 * 256, 1024
    x = rnd(M, K, seed=1, dtype=dt)
    w = rnd(N, K, seed=2, scale=K ** -0.5, dtype=dt)
    bias = rnd(N, seed=3)
    res = rnd(M, N, seed=4, dtype=dt)
    u = rnd(M, N, seed=5, dtype=dt)
    ref = x.float() @ w.float().t()

    def run():
        out = {}
        out["plain"] = ops.linear_fwd(x, w, None)
        out["bias"] = ops.linear_fwd(x, w, bias)
        out["gelu"], out["gelu_pre"] = ops.linear_fwd(x, w, bias, act=ACT_GELU, want_preact=True)
        out["qgelu"] = ops.linear_fwd(x, w, bias, act=ACT_QUICKGELU)
        out["res"] = ops.linear_fwd(x, w, bias, residual=res)
        out["actu"] = ops.linear_dgrad(x, None, w, act=ACT_GELU, u=u)      # x @ w.T * GELU'(u): wt = w is [N,K] = "K x N" here
        torch.cuda.synchronize()
        return out

    try:
        lib.clipx_select_nt_kernel(0)
        base = run()
        lib.clipx_select_nt_kernel(1)
        got = run()
    finally:
        lib.clipx_select_nt_kernel(-1)
    assert relerr(got["plain"], ref) < tol(dt)
    assert relerr(got["gelu_pre"], ref + bias) < tol(dt)
    assert relerr(got["gelu"], act_ref(ACT_GELU, ref + bias)) < tol(dt)
    assert relerr(got["qgelu"], act_ref(ACT_QUICKGELU, ref + bias)) < tol(dt)
    assert relerr(got["res"], ref + bias + res.float()) < tol(dt)
    for k in base:
        # same products, same fp32 accumulation up to ordering, one rounding: a bf16 ulp at most (GELU on the rounded
        # pre-activation in the deferred epilogue: a little more)
        assert relerr(got[k], base[k].float()) < 6e-3, k


@pytest.mark.parametrize("M,N,K", [(200 * 256, 1024, 768), (33 * 256, 1024, 128), (140 * 256 + 77, 512, 512),
                                   (90 * 256, 640, 256), (70 * 256 + 8, 1000, 1024), (800 * 256, 768, 768)])
def test_linear_bf16_pingpong_kernel(M, N, K):
    """The eight-wave ping-pong NT kernel (csrc/gemm_bf16_nt8p.hip) against the one-barrier eight-wave kernel: same tile,
    same fragments, same order of the fp32 accumulation and the same epilogue code, so every output must be BIT-identical;
    and against the fp32 formulas.  Shapes: several tiles per CU (the operand rings run across tile boundaries), partial
    last m-panel, N with a half-empty last n-tile (group B's w rows all beyond N) and N % 256 not a multiple of 8 rows."""
    from colxlip_amd import _lib
    lib = _lib.lib()
    dt = torch.bfloat16
    x = rnd(M, K, seed=1, dtype=dt)
    w = rnd(N, K, seed=2, scale=K ** -0.5, dtype=dt)
    bias = rnd(N, seed=3)
    res = rnd(M, N, seed=4, dtype=dt)
    u = rnd(M, N, seed=5, dtype=dt)

    def run():
        out = {}
        out["plain"] = ops.linear_fwd(x, w, None)
        out["bias"] = ops.linear_fwd(x, w, bias)
        out["gelu"], out["gelu_pre"] = ops.linear_fwd(x, w, bias, act=ACT_GELU, want_preact=True)
        out["res"] = ops.linear_fwd(x, w, bias, residual=res)
        out["actu"] = ops.linear_dgrad(x, None, w, act=ACT_GELU, u=u)
        out["gelu8"], out["gelu8_g"] = ops.linear_fwd(x, w, bias, act=ACT_GELU, want_preact="gelu8")
        out["actu8"] = ops.linear_dgrad(x, None, w, act=ACT_GELU, u=out["gelu8_g"])
        torch.cuda.synchronize()
        return out

    try:
        lib.clipx_select_nt_kernel(0)
        lib.clipx_select_nt_pp(0)
        base = run()
        lib.clipx_select_nt_pp(1)
        got = run()
    finally:
        lib.clipx_select_nt_kernel(-1)
        lib.clipx_select_nt_pp(-1)
    ref = x[:4096].float() @ w.float().t()
    assert relerr(got["plain"][:4096], ref) < tol(dt)
    assert relerr(got["gelu"][:4096], act_ref(ACT_GELU, ref + bias)) < tol(dt)
    for k in base:
        assert torch.equal(got[k], base[k]), (k, (got[k].float() - base[k].float()).abs().max().item())


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("M,N,K", [(64, 128, 128), (256, 64, 64), (1000, 192, 256), (39, 64, 128), (4096, 256, 128),
                                   (20000, 128, 128)])
@pytest.mark.parametrize("beta", [0.0, 1.0])
def test_linear_wgrad(dtype, M, N, K, beta):
    dy = rnd(M, N, seed=1, dtype=dtype)
    x = rnd(M, K, seed=2, dtype=dtype)
    dw0 = rnd(N, K, seed=3)
    ref = dy.float().t() @ x.float() + beta * dw0
    dw = dw0.clone()
    ws = torch.empty(max(ops.linear_wgrad_ws_bytes(dtype, M, N, K), 16), dtype=torch.uint8, device=DEV)
    ops.linear_wgrad(dy, x, dw, beta, ws)
    assert relerr(dw, ref) < (2e-5 if dtype == torch.float32 else 1e-2)
    dw = dw0.clone()
    ops.linear_wgrad(dy, x, dw, beta, None)      # no workspace -> unsplit path
    assert relerr(dw, ref) < (2e-5 if dtype == torch.float32 else 1e-2)
    # bias gradient from the same pass over dy (fp32 sums of the stored values in both modes)
    db0 = rnd(N, seed=4)
    db, dw = db0.clone(), dw0.clone()
    ops.linear_wgrad(dy, x, dw, beta, ws, db=db, beta_b=beta)
    assert relerr(dw, ref) < (2e-5 if dtype == torch.float32 else 1e-2)
    assert relerr(db, dy.float().sum(0) + beta * db0) < 1e-5


@pytest.mark.parametrize("M,N,K", [(512, 2304, 768), (1024, 3072, 768), (777, 768, 3072), (300, 520, 264)])
def test_linear_wgrad_bias_multi_tile(M, N, K):
    """bf16 wgrad with several n- and k-tiles: every (split, k-tile) block contributes bias partials."""
    dy = rnd(M, N, seed=1, dtype=torch.bfloat16)
    x = rnd(M, K, seed=2, dtype=torch.bfloat16)
    dw = torch.empty(N, K, device=DEV)
    db = torch.full((N,), 7.0, device=DEV)
    ws = torch.empty(ops.linear_wgrad_ws_bytes(torch.bfloat16, M, N, K), dtype=torch.uint8, device=DEV)
    ops.linear_wgrad(dy, x, dw, 0.0, ws, db=db, beta_b=0.0)
    assert relerr(dw, dy.float().t() @ x.float()) < 1e-2
    assert relerr(db, dy.float().sum(0)) < 1e-5


@pytest.mark.parametrize("M,N,K", [(204800, 768, 768), (177152 + 40, 512, 2048), (777, 768, 3072), (20000, 256, 512),
                                   (64 * 9 + 1, 2304, 768)])
@pytest.mark.parametrize("beta", [0.0, 1.0])
def test_linear_wgrad_pingpong_kernel(M, N, K, beta):
    """The ping-pong form of the bf16 wgrad kernel against the one-barrier form: same tiles, splits, fragments and order of
    the fp32 accumulation, so dw and the bias gradient must be BIT-identical (and close to the fp32 formula).  Shapes: the
    production ones (many splits), a ragged last 64-row step, splits of four steps, one tile per CU and fewer."""
    from colxlip_amd import _lib
    lib = _lib.lib()
    dy = rnd(M, N, seed=1, dtype=torch.bfloat16)
    x = rnd(M, K, seed=2, dtype=torch.bfloat16)
    dw0, db0 = rnd(N, K, seed=3), rnd(N, seed=4)
    ws = torch.empty(ops.linear_wgrad_ws_bytes(torch.bfloat16, M, N, K), dtype=torch.uint8, device=DEV)
    out = []
    try:
        for which in (0, 1):
            lib.clipx_select_tn_pp(which)
            dw, db = dw0.clone(), db0.clone()
            ops.linear_wgrad(dy, x, dw, beta, ws, db=db, beta_b=beta)
            dw2 = dw0.clone()
            ops.linear_wgrad(dy, x, dw2, beta, None)            # unsplit
            torch.cuda.synchronize()
            out.append((dw, db, dw2))
    finally:
        lib.clipx_select_tn_pp(-1)
    if M <= 20000:
        assert relerr(out[1][0], dy.float().t() @ x.float() + beta * dw0) < 1e-2
    assert relerr(out[1][1], dy.float().sum(0) + beta * db0) < 1e-5
    for a, b in zip(out[0], out[1]):
        assert torch.equal(a, b), (a - b).abs().max().item()


@pytest.mark.parametrize("M,width,mlp", [(25600, 768, 3072), (22784, 512, 2048), (204800, 768, 3072), (1000, 256, 1024),
                                         (640, 768, 3072)])
@pytest.mark.parametrize("beta", [0.0, 1.0])
def test_linear_wgrad_group_equals_single_launches(M, width, mlp, beta):
    """ops.linear_wgrad_group (the four wgrads of a residual block as ONE grid: c_proj, c_fc, out_proj, in_proj over the same M
    rows) against four clipx_linear_wgrad launches: the same tiles and fragments with a different row split, so dw / db agree
    to fp32 summation order (1e-5 of the largest entry) -- and both to the fp32 formula at the small sizes.  Shapes: ViT-B/32
    vision / text blocks at per-GPU batch 512 and 4096, a small block, and a block with few rows (the plan caps the split at
    four 64-row steps).  A shape the grouped kernel does not take (N not a multiple of 256) falls back to single launches."""
    shapes = [(width, mlp, False), (mlp, width, True), (width, width, False), (3 * width, width, True)]       # (N, K, bias grad)
    probs_g, probs_s = [], []
    for i, (N, K, has_b) in enumerate(shapes):
        dy = rnd(M, N, seed=10 + i, dtype=torch.bfloat16)
        x = rnd(M, K, seed=20 + i, dtype=torch.bfloat16)
        dw0, db0 = rnd(N, K, seed=30 + i), rnd(N, seed=40 + i)
        probs_g.append((dy, x, dw0.clone(), beta, db0.clone() if has_b else None, beta))
        probs_s.append((dy, x, dw0.clone(), beta, db0.clone() if has_b else None, beta, dw0, db0))
    ws = torch.empty(ops.linear_wgrad_group_ws_bytes(torch.bfloat16, M, [(n, k) for n, k, _ in shapes]), dtype=torch.uint8, device=DEV)
    ops.linear_wgrad_group(probs_g, ws)
    for dy, x, dw, b, db, bb, _, _ in probs_s:
        ops.linear_wgrad(dy, x, dw, b, ws, db=db, beta_b=bb)
    torch.cuda.synchronize()
    for (dy, x, dwg, _, dbg, _), (_, _, dws, _, dbs, _, dw0, db0) in zip(probs_g, probs_s):
        assert float((dwg - dws).abs().max()) <= 1e-5 * float(dws.abs().max()) + 1e-6
        if dbg is not None:
            assert float((dbg - dbs).abs().max()) <= 1e-5 * float(dbs.abs().max()) + 1e-6
            assert relerr(dbg, dy.float().sum(0) + beta * db0) < 1e-5
        if M <= 25600:
            assert relerr(dwg, dy.float().t() @ x.float() + beta * dw0) < 1e-2
    # fallback: a width the grouped kernel does not take
    dy, x = rnd(300, 192, seed=1, dtype=torch.bfloat16), rnd(300, 320, seed=2, dtype=torch.bfloat16)
    dw = torch.zeros(192, 320, device=DEV)
    ws2 = torch.empty(max(ops.linear_wgrad_group_ws_bytes(torch.bfloat16, 300, [(192, 320)]), 256), dtype=torch.uint8, device=DEV)
    ops.linear_wgrad_group([(dy, x, dw, 0.0, None, 0.0)], ws2)
    assert relerr(dw, dy.float().t() @ x.float()) < 1e-2


@pytest.mark.parametrize("M", [25600 + 37, 999, 204800 - 5, 63])
def test_linear_wgrad_group_ragged_rows_mixed_accumulation(M):
    """Advisor finding (round 3): the grouped wgrad's slab layout and reduce jobs against the per-problem path with M NOT a
    multiple of the rows per split (and below one 64-row ring step), beta = 0 and beta = 1 MIXED inside one call (two of the four
    problems accumulate into existing gradients, as under gradient accumulation with a late-created .grad), bias gradients
    present on two problems with their own mixed beta, absent on the others."""
    width, mlp = 512, 2048
    shapes = [(width, mlp, False, 1.0, 0.0), (mlp, width, True, 0.0, 1.0), (width, width, False, 0.0, 0.0), (3 * width, width, True, 1.0, 0.0)]
    probs_g, probs_s = [], []
    for i, (N, K, has_b, beta, beta_b) in enumerate(shapes):
        dy = rnd(M, N, seed=50 + i, dtype=torch.bfloat16)
        x = rnd(M, K, seed=60 + i, dtype=torch.bfloat16)
        dw0, db0 = rnd(N, K, seed=70 + i), rnd(N, seed=80 + i)
        probs_g.append((dy, x, dw0.clone(), beta, db0.clone() if has_b else None, beta_b))
        probs_s.append((dy, x, dw0.clone(), beta, db0.clone() if has_b else None, beta_b, dw0, db0))
    ws = torch.empty(ops.linear_wgrad_group_ws_bytes(torch.bfloat16, M, [(n, k) for n, k, *_ in shapes]), dtype=torch.uint8, device=DEV)
    ops.linear_wgrad_group(probs_g, ws)
    for dy, x, dw, b, db, bb, _, _ in probs_s:
        ops.linear_wgrad(dy, x, dw, b, ws, db=db, beta_b=bb)
    torch.cuda.synchronize()
    for (dy, x, dwg, beta, dbg, beta_b), (_, _, dws, _, dbs, _, dw0, db0) in zip(probs_g, probs_s):
        assert float((dwg - dws).abs().max()) <= 1e-5 * float(dws.abs().max()) + 1e-6
        if M <= 30000:
            assert relerr(dwg, dy.float().t() @ x.float() + beta * dw0) < 1e-2
        if dbg is not None:
            assert float((dbg - dbs).abs().max()) <= 1e-5 * float(dbs.abs().max()) + 1e-6
            assert relerr(dbg, dy.float().sum(0) + beta_b * db0) < 1e-5


def _dequant_e4m3(q8, expo):
    return q8.view(torch.float8_e4m3fn).float() * torch.exp2(expo.float())[:, None]


@pytest.mark.parametrize("M,K", [(1000, 1280), (257, 5120), (64, 128), (300, 8192)])
def test_quant_rows_e4m3(M, K):
    """Activation rows for the fp8 MFMA GEMM: exponent rule (smallest e with max|x| 2^-e <= 448) and the hardware's e4m3
    rounding, against torch's float8_e4m3fn cast of the scaled row -- bit for bit."""
    x = (rnd(M, K, seed=1) * torch.exp2(torch.randint(-6, 7, (M, 1), device=DEV).float())).bfloat16()
    x[3] = 0
    x8, xe = ops.quant_rows_e4m3(x)
    amax = x.float().abs().amax(1)
    e_ref = torch.ceil(torch.log2(amax.clamp_min(1e-30) / 448.0)).to(torch.int32)
    e_ref[amax == 0] = 0
    assert torch.equal(xe, e_ref)
    ref8 = (x.float() * torch.exp2(-xe.float())[:, None]).to(torch.float8_e4m3fn).view(torch.uint8)
    assert torch.equal(x8 & 0x7f, ref8 & 0x7f) and torch.equal((x8 >> 7)[x8 & 0x7f != 0], (ref8 >> 7)[ref8 & 0x7f != 0])


@pytest.mark.parametrize("rows,width", [(1000, 1280), (257, 768), (77, 512), (4099, 1024), (33, 256)])
def test_layernorm_fwd_q8(rows, width):
    """LayerNorm forward with the e4m3 row quantiser fused in: y / mean / rstd equal the plain kernel's bit for bit, and the
    fp8 bytes + exponents equal a quant_rows_e4m3 pass over that y bit for bit."""
    x = (rnd(rows, width, seed=1) * torch.exp2((torch.arange(rows, device=DEV) % 9 - 4).float())[:, None]).bfloat16()
    gamma = 1 + 0.1 * rnd(width, seed=2)
    beta = 0.1 * rnd(width, seed=3)
    y0, m0, r0 = ops.layernorm_fwd(x, gamma, beta)
    y, m, r, y8, ye = ops.layernorm_fwd_q8(x, gamma, beta)
    assert torch.equal(y, y0) and torch.equal(m, m0) and torch.equal(r, r0)
    q8, qe = ops.quant_rows_e4m3(y0)
    assert torch.equal(ye, qe) and torch.equal(y8, q8)


@pytest.mark.parametrize("M,N,K", [(150 * 256, 1280, 1280), (33 * 256 + 40, 3840, 1280), (140 * 256, 1280, 5120),
                                   (200 * 256, 1000, 256)])
def test_linear_fwd_fp8_mfma(M, N, K):
    """fp8 x fp8 forward linear on v_mfma_f32_16x16x128_f8f6f4 (csrc/gemm_fp8_nt8p.hip) against the fp64 product of the
    DEQUANTISED operands: the e4m3 products are exact and the sums fp32, so what is left is the bf16 rounding of the output
    (and of the pre-activation in front of the GELU).  ViT-H/14's shapes at a batch that gives whole 256x256 tiles, a partial
    last m-panel, a ragged N, several tiles per CU."""
    dt = torch.bfloat16
    x = (rnd(M, K, seed=1) * torch.exp2((torch.arange(M, device=DEV) % 7 - 3).float())[:, None]).to(dt)
    w = rnd(N, K, seed=2, scale=K ** -0.5)
    bias = rnd(N, seed=3)
    res = rnd(M, N, seed=4, dtype=dt)
    we = torch.empty(N, dtype=torch.int32, device=DEV)
    w8 = torch.empty(N, K, dtype=torch.uint8, device=DEV)
    ops.quant_weight_e4m3(w, we, w8, None, None)
    x8, xe = ops.quant_rows_e4m3(x)
    rows = slice(0, 2048)
    ref = _dequant_e4m3(x8[rows], xe[rows]).double() @ _dequant_e4m3(w8, we).double().t()
    y = ops.linear_fwd_fp8(x8, xe, w8, we)
    e_ = relerr(y[rows], ref)
    assert e_ < tol(dt), ("relerr(y[rows], ref)", e_)
    tail = slice(M - 300, M)
    ref_t = _dequant_e4m3(x8[tail], xe[tail]).double() @ _dequant_e4m3(w8, we).double().t()
    e_ = relerr(y[tail], ref_t)
    assert e_ < tol(dt), ("relerr(y[tail], ref_t)", e_)
    yb = ops.linear_fwd_fp8(x8, xe, w8, we, bias)
    e_ = relerr(yb[rows], ref + bias.double())
    assert e_ < tol(dt), ("relerr(yb[rows], ref + bias.double())", e_)
    h, u = ops.linear_fwd_fp8(x8, xe, w8, we, bias, act=ACT_GELU, want_preact=True)
    e_ = relerr(u[rows], ref + bias.double())
    assert e_ < tol(dt), ("relerr(u[rows], ref + bias.double())", e_)
    e_ = relerr(h[rows], act_ref(ACT_GELU, (ref + bias.double()).float()))
    assert e_ < tol(dt), ("relerr(h[rows], act_ref(ACT_GELU, (ref + bias.double()).floa", e_)
    # GELU' kept on eight bits instead of the pre-activation (csrc/gemm_epi.h G8_*): same y, the byte decodes to GELU'(u)
    h8, g8 = ops.linear_fwd_fp8(x8, xe, w8, we, bias, act=ACT_GELU, want_preact="gelu8")
    assert torch.equal(h8, h)
    uu_ = (ref + bias.double())
    exact_g = 0.5 * (1 + torch.erf(uu_ / math.sqrt(2))) + uu_ * torch.exp(-uu_ * uu_ / 2) / math.sqrt(2 * math.pi)
    e_ = float((-0.13 + 0.005 * g8[rows].double() - exact_g).abs().max())
    assert e_ < 0.0025 + 6e-4, ("8-bit GELU' factor", e_)
    yr = ops.linear_fwd_fp8(x8, xe, w8, we, bias, residual=res)
    e_ = relerr(yr[rows], ref + bias.double() + res[rows].double())
    assert e_ < tol(dt), ("relerr(yr[rows], ref + bias.double() + res[rows].double())", e_)
    # dgrad form of the same kernel (reduction over N): dx = dy8 @ wt8^T with the rows of the [K,N] copy quantised, x GELU'(u)
    if N % 128 == 0:
        dy = (rnd(M, N, seed=6) * torch.exp2((torch.arange(M, device=DEV) % 11 - 8).float())[:, None]).to(dt)
        wt16 = w.t().contiguous().to(dt)
        uu = rnd(M, K, seed=7, dtype=dt)
        d8, de = ops.quant_rows_e4m3(dy)
        wt8, wte = ops.quant_rows_e4m3(wt16)
        refd = _dequant_e4m3(d8[rows], de[rows]).double() @ _dequant_e4m3(wt8, wte).double().t()
        dx = ops.linear_dgrad_fp8(d8, de, wt8, wte)
        e_ = relerr(dx[rows], refd)
        assert e_ < tol(dt), ("relerr(dx[rows], refd)", e_)
        gq = torch.randint(0, 256, (M, K), dtype=torch.uint8, device=DEV)
        dx8 = ops.linear_dgrad_fp8(d8, de, wt8, wte, act=ACT_GELU, u=gq)
        e_ = relerr(dx8[rows], refd * (-0.13 + 0.005 * gq[rows].double()))
        assert e_ < tol(dt), ("dgrad x 8-bit factor", e_)
        dxa = ops.linear_dgrad_fp8(d8, de, wt8, wte, act=ACT_GELU, u=uu)
        e_ = relerr(dxa[rows], refd * act_grad_ref(ACT_GELU, uu[rows].float()).double())
        assert e_ < tol(dt), ("relerr(dxa[rows], refd * act_grad_ref(ACT_GELU, uu[rows]))", e_)
    # and against the bf16 kernel on the dequantised operands (exact in bf16): same products, same fp32 sums up to their order
    xd, wd = _dequant_e4m3(x8, xe).to(dt), _dequant_e4m3(w8, we).to(dt)
    y16 = ops.linear_fwd(xd, wd, None)
    e_ = relerr(y, y16.float())
    assert e_ < 5e-3, ("relerr(y, y16.float())", e_)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_colsum(dtype):
    a = rnd(1000, 768, seed=1, dtype=dtype)
    out0 = rnd(768, seed=2)
    ws = torch.empty(ops.colsum_ws_bytes(1000, 768), dtype=torch.uint8, device=DEV)
    out = out0.clone()
    ops.colsum(a, out, 1.0, ws)
    assert relerr(out, a.float().sum(0) + out0) < 1e-5
    ops.colsum(a, out, 0.0, ws)
    assert relerr(out, a.float().sum(0)) < 1e-5


# ------------------------------------------------------------------ LayerNorm
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("rows,width", [(100, 64), (257, 768), (77, 512), (33, 1280)])
def test_layernorm(dtype, rows, width):
    x = rnd(rows, width, seed=1, dtype=dtype)
    gamma = 1 + 0.1 * rnd(width, seed=2)
    beta = 0.1 * rnd(width, seed=3)
    dy = rnd(rows, width, seed=4, dtype=dtype)
    res = rnd(rows, width, seed=5, dtype=dtype)
    xf = x.float().detach().clone().requires_grad_(True)
    gf, bf = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    y_ref = torch.nn.functional.layer_norm(xf, (width,), gf, bf, 1e-5)
    y_ref.backward(dy.float())
    y, mean, rstd = ops.layernorm_fwd(x, gamma, beta)
    assert relerr(y, y_ref) < (1e-5 if dtype == torch.float32 else 1e-2)
    ws = torch.empty(ops.layernorm_ws_bytes(width), dtype=torch.uint8, device=DEV)
    dx = ops.layernorm_bwd(dy, x, gamma, mean, rstd, ws, dx_res=res)
    dgamma = torch.zeros(width, device=DEV)
    dbeta = torch.ones(width, device=DEV)
    cs = torch.empty(width, device=DEV)
    ops.layernorm_bwd_finish(width, ws, dgamma, None, None, 0.0)
    ops.layernorm_bwd_finish(width, ws, None, dbeta, None, 1.0)
    ops.layernorm_bwd_finish(width, ws, None, None, cs, 0.0)
    t = 2e-5 if dtype == torch.float32 else 1.5e-2
    assert relerr(dx, xf.grad + res.float()) < t
    assert relerr(dgamma, gf.grad) < t
    assert relerr(dbeta, bf.grad + 1.0) < t
    assert relerr(cs, dx.float().sum(0)) < (1e-4 if dtype == torch.float32 else 2e-2)


def test_layernorm_row_index():
    x = rnd(60, 128, seed=1)
    gamma, beta = 1 + 0.1 * rnd(128, seed=2), 0.1 * rnd(128, seed=3)
    idx = torch.tensor([3, 17, 59, 0], dtype=torch.int32, device=DEV)
    y, mean, rstd = ops.layernorm_fwd(x, gamma, beta, rows=4, row_index=idx)
    ref = torch.nn.functional.layer_norm(x[idx.long()], (128,), gamma, beta, 1e-5)
    assert relerr(y, ref) < 1e-5
    dy = rnd(4, 128, seed=4)
    ws = torch.empty(ops.layernorm_ws_bytes(128), dtype=torch.uint8, device=DEV)
    dx = torch.zeros_like(x)
    ops.layernorm_bwd(dy, x, gamma, mean, rstd, ws, dx_out=dx, row_index=idx)
    xf = x.clone().requires_grad_(True)
    torch.nn.functional.layer_norm(xf[idx.long()], (128,), gamma, beta, 1e-5).backward(dy)
    assert relerr(dx, xf.grad) < 2e-5


# ------------------------------------------------------------------ attention
def attn_ref(qkv, batch, L, heads, causal):
    d = qkv.shape[-1] // 3
    hd = d // heads
    q, k, v = qkv.float().view(batch, L, 3, heads, hd).permute(2, 0, 3, 1, 4)
    s = q @ k.transpose(-1, -2) * hd ** -0.5
    if causal:
        s = s + torch.triu(torch.full((L, L), float("-inf"), device=qkv.device), 1)
    o = torch.softmax(s, -1) @ v
    return o.permute(0, 2, 1, 3).reshape(batch * L, d)


@pytest.mark.parametrize("dtype,hd", [(torch.float32, 64), (torch.float32, 32), (torch.float32, 80), (torch.bfloat16, 64)])
@pytest.mark.parametrize("L,causal", [(50, False), (77, True), (5, False), (17, True), (64, True), (128, False), (197, False)])
def test_attention(dtype, hd, L, causal):
    batch, heads = 3, 2
    d = heads * hd
    qkv = rnd(batch * L, 3 * d, seed=1, scale=1.0, dtype=dtype)
    dout = rnd(batch * L, d, seed=2, dtype=dtype)
    qf = qkv.float().detach().clone().requires_grad_(True)
    o_ref = attn_ref(qf, batch, L, heads, causal)
    o_ref.backward(dout.float())
    o = ops.attention_fwd(qkv, batch, L, heads, causal)
    dqkv = ops.attention_bwd(qkv, dout, batch, L, heads, causal)
    t = 1e-5 if dtype == torch.float32 else 2e-2
    assert relerr(o, o_ref) < t
    assert relerr(dqkv, qf.grad) < (2e-5 if dtype == torch.float32 else 3e-2)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("hd,L,causal", [(64, 577, False), (80, 257, False), (64, 300, True), (80, 77, True), (128, 130, False),
                                         (32, 50, False), (64, 700, True)])
def test_attention_generic_tiled(dtype, hd, L, causal):
    """Shapes outside the whole-sequence kernels (ViT-L/14-336: 577 tokens, ViT-H/14: head dim 80, long fp32
    sequences) take the tiled online-softmax kernels."""
    batch, heads = 2, 2
    d = heads * hd
    qkv = rnd(batch * L, 3 * d, seed=1, scale=1.0, dtype=dtype)
    dout = rnd(batch * L, d, seed=2, dtype=dtype)
    qf = qkv.float().detach().clone().requires_grad_(True)
    o_ref = attn_ref(qf, batch, L, heads, causal)
    o_ref.backward(dout.float())
    o = ops.attention_fwd(qkv, batch, L, heads, causal)
    dqkv = ops.attention_bwd(qkv, dout, batch, L, heads, causal)
    assert relerr(o, o_ref) < (1e-5 if dtype == torch.float32 else 2e-2)
    assert relerr(dqkv, qf.grad) < (3e-5 if dtype == torch.float32 else 3e-2)


@pytest.mark.parametrize("L,causal", [(129, False), (130, True), (160, True), (197, False), (224, False), (225, False), (256, True),
                                      (257, False), (320, False), (321, True), (400, True), (577, False), (608, False), (608, True)])
def test_attention_bf16_long_mfma(L, causal):
    """128 < L <= 608 at head dim 64 in bf16 (two 8-wave blocks per CU up to L = 320, one 16-wave block beyond): the online-softmax MFMA kernels (K, V of a (sample, head) whole in LDS,
    scores chunk-wise) -- odd tile counts, partial last pair, chunk tails, causal early exit."""
    batch, heads, hd = 2, 3, 64
    d = heads * hd
    for scale in (1.0, 3.0):                  # 3.0: sharp softmax, the running maximum moves between chunks
        qkv = rnd(batch * L, 3 * d, seed=1, scale=scale, dtype=torch.bfloat16)
        dout = rnd(batch * L, d, seed=2, dtype=torch.bfloat16)
        qf = qkv.float().detach().clone().requires_grad_(True)
        o_ref = attn_ref(qf, batch, L, heads, causal)
        o_ref.backward(dout.float())
        o = ops.attention_fwd(qkv, batch, L, heads, causal)
        dqkv = ops.attention_bwd(qkv, dout, batch, L, heads, causal)
        assert torch.isfinite(o.float()).all() and torch.isfinite(dqkv.float()).all()
        assert relerr(o, o_ref) < 2e-2
        assert relerr(dqkv, qf.grad) < 3e-2


@pytest.mark.parametrize("L,causal", [(257, False), (50, False), (77, True), (288, True), (33, False), (100, True)])
def test_attention_bf16_head_dim_80_mfma(L, causal):
    """Head dim 80 in bf16 (ViT-H/14: 257 tokens): LDS rows padded to 128 elements, three k-slices, five output tiles, the
    fifth stored separately."""
    batch, heads, hd = 2, 3, 80
    d = heads * hd
    for scale in (1.0, 3.0):
        qkv = rnd(batch * L, 3 * d, seed=1, scale=scale, dtype=torch.bfloat16)
        dout = rnd(batch * L, d, seed=2, dtype=torch.bfloat16)
        qf = qkv.float().detach().clone().requires_grad_(True)
        o_ref = attn_ref(qf, batch, L, heads, causal)
        o_ref.backward(dout.float())
        o = ops.attention_fwd(qkv, batch, L, heads, causal)
        dqkv = ops.attention_bwd(qkv, dout, batch, L, heads, causal)
        assert torch.isfinite(o.float()).all() and torch.isfinite(dqkv.float()).all()
        assert relerr(o, o_ref) < 2e-2
        assert relerr(dqkv, qf.grad) < 3e-2


@pytest.mark.parametrize("hd,L,causal", [(80, 257, False), (80, 288, True), (80, 33, False), (64, 577, False), (64, 256, True),
                                         (64, 225, False), (64, 608, True), (64, 197, False), (64, 130, True)])
def test_attention_bf16_lse_handover(hd, L, causal):
    """clipx_attention_fwd_lse / _bwd_lse (the online-softmax kernels): the forward's log-sum-exp equals the fp32 formula
    (log2 domain), its output is bit-identical to the plain forward's, and the backward that takes (out, lse) -- delta from
    rowsum(dout * out) instead of a sweep over the keys -- agrees with the fp32 reference to the same bound as the two-sweep
    backward, and with the two-sweep backward to within bf16 rounding of `out`.  Shapes without the hand-over return None."""
    batch, heads = 2, 3
    d = heads * hd
    for scale in (1.0, 3.0):
        qkv = rnd(batch * L, 3 * d, seed=1, scale=scale, dtype=torch.bfloat16)
        dout = rnd(batch * L, d, seed=2, dtype=torch.bfloat16)
        qf = qkv.float().detach().clone().requires_grad_(True)
        o_ref = attn_ref(qf, batch, L, heads, causal)
        o_ref.backward(dout.float())
        o, lse = ops.attention_fwd(qkv, batch, L, heads, causal, want_lse=True)
        assert lse is not None and lse.shape == (batch * heads, L)
        assert torch.equal(o, ops.attention_fwd(qkv, batch, L, heads, causal))
        q, k, _ = qkv.float().view(batch, L, 3, heads, hd).permute(2, 0, 3, 1, 4)
        sc = q @ k.transpose(-1, -2) * hd ** -0.5
        if causal:
            sc = sc + torch.triu(torch.full((L, L), float("-inf"), device=DEV), 1)
        want = torch.logsumexp(sc, -1).reshape(batch * heads, L) * 1.4426950408889634
        assert float((lse - want).abs().max()) < 2e-3 * max(1.0, float(want.abs().max()))
        dq_lse = ops.attention_bwd(qkv, dout, batch, L, heads, causal, out=o, lse=lse)
        dq_two = ops.attention_bwd(qkv, dout, batch, L, heads, causal)
        assert torch.isfinite(dq_lse.float()).all()
        assert relerr(dq_lse, qf.grad) < 3e-2
        assert relerr(dq_lse, dq_two) < 1.5e-2
    if not causal:
        # every score far below zero (log-sum-exp ~ -290 in the log2 domain): the zero rows that pad K in LDS would give
        # P = exp2(0 + 290) = inf without the cut of the padded keys in the mask-free backward path
        qkv3 = torch.zeros(batch, L, 3, heads, hd, device=DEV)
        qkv3[:, :, 0] = -26.0
        qkv3[:, :, 1] = 1.0
        qkv3[:, :, 2] = rnd(batch * L, d, seed=5).view(batch, L, heads, hd)
        qkv = qkv3.reshape(batch * L, 3 * d).to(torch.bfloat16)
        qf = qkv.float().detach().clone().requires_grad_(True)
        o_ref = attn_ref(qf, batch, L, heads, causal)
        o_ref.backward(dout.float())
        o, lse = ops.attention_fwd(qkv, batch, L, heads, causal, want_lse=True)
        assert float(lse.max()) < -250.0
        dq_lse = ops.attention_bwd(qkv, dout, batch, L, heads, causal, out=o, lse=lse)
        assert torch.isfinite(o.float()).all() and torch.isfinite(dq_lse.float()).all()
        assert relerr(o, o_ref) < 2e-2
        dv_ref = qf.grad.view(batch * L, 3, d)[:, 2]
        assert relerr(dq_lse.view(batch * L, 3, d)[:, 2], dv_ref) < 3e-2       # (dq, dk are ~0 here: uniform attention)
    small = rnd(2 * 50, 3 * 128, seed=3, dtype=torch.bfloat16)
    assert ops.attention_fwd(small, 2, 50, 2, False, want_lse=True)[1] is None          # whole-sequence kernel: nothing to hand over
    assert ops.attention_fwd(small.float(), 2, 50, 2, False, want_lse=True)[1] is None


def test_attention_bf16_sharp_softmax():
    """large-magnitude scores: exercises the max-subtraction / masked -inf paths."""
    batch, heads, L, hd = 2, 2, 77, 64
    qkv = rnd(batch * L, 3 * heads * hd, seed=5, scale=3.0, dtype=torch.bfloat16)
    o = ops.attention_fwd(qkv, batch, L, heads, True)
    assert torch.isfinite(o.float()).all()
    assert relerr(o, attn_ref(qkv, batch, L, heads, True)) < 3e-2


# ------------------------------------------------------------------ embeddings
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("P,size", [(16, 32), (32, 224), (14, 28)])
def test_patchify_assemble(dtype, P, size):
    b = 3
    img = rnd(b, 3, size, size, seed=1)
    K = 3 * P * P
    Kp = K if dtype == torch.float32 else (K + 63) // 64 * 64
    patches = ops.patchify(img, P, Kp, dtype)
    G = size // P
    ref = img.reshape(b, 3, G, P, G, P).permute(0, 2, 4, 1, 3, 5).reshape(b * G * G, K)
    assert relerr(patches[:, :K], ref) < (1e-7 if dtype == torch.float32 else 1e-2)
    if Kp > K:
        assert float(patches[:, K:].float().abs().max()) == 0.0
    width = 64
    tok = rnd(b * G * G, width, seed=2, dtype=dtype)
    cls, pos = rnd(width, seed=3), rnd(G * G + 1, width, seed=4)
    x0 = ops.vision_assemble(tok, cls, pos, b, G * G + 1)
    ref = torch.cat([cls.view(1, 1, -1).expand(b, 1, width), tok.float().view(b, G * G, width)], 1) + pos
    assert relerr(x0, ref.reshape(-1, width)) < (1e-6 if dtype == torch.float32 else 1e-2)
    dx0 = rnd(b * (G * G + 1), width, seed=5, dtype=dtype)
    dpos = torch.ones(G * G + 1, width, device=DEV)
    dcls = torch.ones(width, device=DEV)
    dtok = ops.vision_assemble_bwd(dx0, b, G * G + 1, dpos, dcls, 1.0)
    d3 = dx0.float().view(b, G * G + 1, width)
    assert relerr(dtok, d3[:, 1:].reshape(-1, width)) < 1e-6
    assert relerr(dpos, d3.sum(0) + 1.0) < 1e-5
    assert relerr(dcls, d3[:, 0].sum(0) + 1.0) < 1e-5
    ops.vision_assemble_bwd(dx0, b, G * G + 1, dpos, dcls, 0.0)
    assert relerr(dpos, d3.sum(0)) < 1e-5


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_text_embed(dtype):
    b, L, width, vocab = 5, 77, 128, 300
    g = torch.Generator().manual_seed(0)
    text = torch.randint(0, vocab, (b, L), generator=g).to(DEV)
    text[:, 40:] = 0
    table, pos = rnd(vocab, width, seed=1), rnd(L, width, seed=2)
    x0 = ops.text_embed(text, table, pos, dtype)
    ref = table[text] + pos
    assert relerr(x0, ref.reshape(-1, width)) < (1e-6 if dtype == torch.float32 else 1e-2)
    dx0 = rnd(b * L, width, seed=3, dtype=dtype)
    dx0.view(b, L, width)[:, 50:] = 0          # rows behind EOT carry exactly-zero gradient
    dtable = torch.zeros(vocab, width, device=DEV)
    dpos = torch.zeros(L, width, device=DEV)
    ops.text_embed_bwd(text, dx0, dtable, dpos, 0.0)
    ref_t = torch.zeros(vocab, width, device=DEV).index_add_(0, text.reshape(-1), dx0.float())
    assert relerr(dtable, ref_t) < 1e-5
    assert relerr(dpos, dx0.float().view(b, L, width).sum(0)) < 1e-5
    idx = ops.eot_index(text)
    assert torch.equal(idx.long(), torch.arange(b, device=DEV) * L + text.argmax(-1))
    assert torch.equal(ops.stride_index(b, 50, DEV).long(), torch.arange(b, device=DEV) * 50)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_gather_scatter_rows(dtype):
    src = rnd(300, 128, seed=1, dtype=dtype)
    idx = torch.randperm(300, generator=torch.Generator().manual_seed(2))[:37].to(torch.int32).to(DEV)
    got = ops.gather_rows(src, idx)
    assert torch.equal(got, src[idx.long()])
    dense = ops.scatter_rows(got, idx, 300)
    want = torch.zeros_like(src)
    want[idx.long()] = src[idx.long()]
    assert torch.equal(dense, want)
    acc = src.clone()
    ops.scatter_add_rows(got, idx, acc)
    want2 = src.float()
    want2[idx.long()] += src[idx.long()].float()
    assert torch.equal(acc.float(), want2.to(dtype).float())


# ------------------------------------------------------------------ packed ("unpadded") text rows
def _captions(batch, L, vocab, seed, min_len=2):
    """token ids with one EOT (= vocab-1, the maximum id) per row, zeros behind it (the reference tokenizer's layout)."""
    g = torch.Generator().manual_seed(seed)
    text = torch.randint(1, vocab - 2, (batch, L), generator=g)
    eot = torch.randint(min_len - 1, L, (batch,), generator=g)
    eot[0], eot[batch - 1] = L - 1, min_len - 1            # the extremes are always present
    pos = torch.arange(L).unsqueeze(0)
    text = torch.where(pos < eot.unsqueeze(1), text, torch.zeros_like(text))
    text[torch.arange(batch), eot] = vocab - 1
    return text, eot + 1


@pytest.mark.parametrize("batch", [3, 64, 1000, 4099])
def test_text_layout_kernel(batch):
    L, vocab = 77, 1000
    text, lens = _captions(batch, L, vocab, seed=batch)
    lay = ops.TextLayout(text.to(DEV), vocab)
    R = int(lens.sum())
    Rp = (R + 255) // 256 * 256
    fill = []
    r = R
    while r < Rp:
        fill.append(min(L, Rp - r))
        r += fill[-1]
    all_len = torch.cat([lens, torch.tensor(fill, dtype=lens.dtype)])
    assert (lay.rows_live, lay.rows, lay.nseq, lay.longest) == (R, Rp, batch + len(fill), int(all_len.max()))
    cu = torch.cat([torch.zeros(1, dtype=torch.long), all_len.cumsum(0)])
    assert torch.equal(lay.cu[:lay.nseq + 1].cpu().long(), cu)
    cls = (all_len > 32).long() + (all_len > 64).long()
    want_order = torch.cat([torch.nonzero(cls == c).flatten() for c in range(3)])       # stable bucket sort
    assert torch.equal(lay.order[:lay.nseq].cpu().long(), want_order)
    assert [c for _, c, _ in lay.buckets] == [int((cls == c).sum()) for c in range(3) if int((cls == c).sum()) > 0]
    tok = torch.cat([text[s, :lens[s]] for s in range(batch)] + [torch.zeros(f, dtype=text.dtype) for f in fill])
    posi = torch.cat([torch.arange(int(n)) for n in all_len])
    assert torch.equal(lay.row_tok[:Rp].cpu().long(), tok) and torch.equal(lay.row_pos[:Rp].cpu().long(), posi)
    assert torch.equal(lay.eot_rows.cpu().long(), cu[1:batch + 1] - 1)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_text_embed_packed(dtype):
    b, L, width, vocab = 37, 77, 128, 300
    text, lens = _captions(b, L, vocab, seed=4)
    text = text.to(DEV)
    lay = ops.TextLayout(text, vocab)
    table, pos = rnd(vocab, width, seed=1), rnd(L, width, seed=2)
    x0 = ops.text_embed_packed(lay, table, pos, dtype)
    dense = (table[text] + pos)
    for s in (0, 1, b - 1):
        r0 = int(lay.cu[s])
        assert relerr(x0[r0:r0 + int(lens[s])], dense[s, :int(lens[s])]) < (1e-6 if dtype == torch.float32 else 1e-2)
    dx0 = rnd(lay.rows, width, seed=3, dtype=dtype)
    dx0[lay.rows_live:] = 0                          # filler sequences receive an exactly-zero gradient
    dtable = torch.zeros(vocab, width, device=DEV)
    dpos = torch.zeros(L, width, device=DEV)
    ops.text_embed_packed_bwd(lay, dx0, dtable, dpos, 0.0)
    ref_t = torch.zeros(vocab, width, device=DEV).index_add_(0, lay.row_tok[:lay.rows].long(), dx0.float())
    ref_p = torch.zeros(L, width, device=DEV).index_add_(0, lay.row_pos[:lay.rows].long(), dx0.float())
    assert relerr(dtable, ref_t) < 1e-5 and relerr(dpos, ref_p) < 1e-5
    ops.text_embed_packed_bwd(lay, dx0, dtable, dpos, 1.0)          # accumulate
    assert relerr(dpos, 2 * ref_p) < 1e-5


@pytest.mark.parametrize("packed", [False, True])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_text_embed_bwd_token_sums(packed, dtype):
    """The token-embedding gradient at the magnitudes of training (columns of 1e-9 .. 1e-3 per row; the EOT token on every
    caption, the pad token on ~half the dense rows) against a float64 sum.  The 64-bit fixed-point sum is exact up to half a
    step of 2^-(58 - ceil(log2 rows)) per contribution and is rounded to fp32 once; a second run gives the same bits; a NaN, an
    inf and a contribution of 1e7 (beyond the fixed-point range) still reach the gradient."""
    b, L, width, vocab = 300, 77, 128, 300
    text, _ = _captions(b, L, vocab, seed=9)
    text = text.to(DEV)
    if packed:
        lay = ops.TextLayout(text, vocab)
        rows, tok = lay.rows, lay.row_tok[:lay.rows].long()
    else:
        rows, tok = b * L, text.reshape(-1)
    g = torch.Generator().manual_seed(5)
    mag = 10.0 ** torch.empty(1, width).uniform_(-9, -3, generator=g)
    dx0 = (torch.randn(rows, width, generator=g) * mag).to(dtype).to(DEV)
    if packed:
        dx0[lay.rows_live:] = 0

    def run(d):
        dtable = torch.zeros(vocab, width, device=DEV)
        dpos = torch.zeros(L, width, device=DEV)
        if packed:
            ops.text_embed_packed_bwd(lay, d, dtable, dpos, 0.0)
        else:
            ops.text_embed_bwd(text, d, dtable, dpos, 0.0)
        return dtable

    got = run(dx0)
    assert torch.equal(got, run(dx0))
    ref = torch.zeros(vocab, width, dtype=torch.float64, device=DEV).index_add_(0, tok, dx0.double())
    count = torch.zeros(vocab, dtype=torch.float64, device=DEV).index_add_(0, tok, torch.ones(rows, dtype=torch.float64,
                                                                                          device=DEV)).unsqueeze(1)
    step = 2.0 ** -(58 - math.ceil(math.log2(rows)))
    err = (got.double() - ref).abs()
    assert bool((err <= ref.abs() * 2.0 ** -23 + count * step / 2).all()), float((err - ref.abs() * 2.0 ** -23).max())

    special = dx0.clone()
    special[0, 0], special[1, 1], special[2, 2] = float("nan"), float("inf"), 1e7
    got = run(special)
    ref = torch.zeros(vocab, width, dtype=torch.float64, device=DEV).index_add_(0, tok, special.double())
    assert torch.isnan(got[tok[0], 0]) and torch.isinf(got[tok[1], 1]) and got[tok[1], 1] > 0
    assert abs(float(got[tok[2], 2]) - float(ref[tok[2], 2])) <= 1e-6 * abs(float(ref[tok[2], 2]))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("batch", [5, 300])
def test_packed_attention_equals_padded(dtype, batch):
    """Causal attention over packed rows (one launch per length bucket, fewer key tiles for short captions) against the
    dense kernel on the same captions padded to 77 rows: rows 0..EOT must agree."""
    L, heads, hd, vocab = 77, 2, 64, 500
    d = heads * hd
    text, lens = _captions(batch, L, vocab, seed=7 + batch)
    lay = ops.TextLayout(text.to(DEV), vocab)
    qkv_p = rnd(lay.rows, 3 * d, seed=1, dtype=dtype)
    dout_p = rnd(lay.rows, d, seed=2, dtype=dtype)
    dout_p[lay.rows_live:] = 0
    qkv_d = torch.zeros(batch, L, 3 * d, device=DEV, dtype=dtype)
    dout_d = torch.zeros(batch, L, d, device=DEV, dtype=dtype)
    cu = lay.cu.cpu().tolist()
    for s in range(batch):
        n = int(lens[s])
        qkv_d[s, :n] = qkv_p[cu[s]:cu[s] + n]
        dout_d[s, :n] = dout_p[cu[s]:cu[s] + n]
    o_p = ops.attention_packed_fwd(qkv_p, lay, heads, True)
    dq_p = ops.attention_packed_bwd(qkv_p, dout_p, lay, heads, True)
    o_d = ops.attention_fwd(qkv_d.view(batch * L, 3 * d), batch, L, heads, True).view(batch, L, d)
    dq_d = ops.attention_bwd(qkv_d.view(batch * L, 3 * d), dout_d.view(batch * L, d), batch, L, heads, True).view(batch, L, 3 * d)
    t = 1e-6 if dtype == torch.float32 else 1e-2
    for s in range(batch):
        n = int(lens[s])
        assert relerr(o_p[cu[s]:cu[s] + n], o_d[s, :n]) < t, s
        assert relerr(dq_p[cu[s]:cu[s] + n], dq_d[s, :n]) < t, s
    assert float(dq_p[lay.rows_live:].float().abs().max()) == 0.0        # fillers: exactly zero


@pytest.mark.parametrize("hd,L,causal", [(64, 50, False), (64, 197, False), (64, 577, False), (80, 257, False), (64, 77, True),
                                         (64, 640, False), (80, 33, True)])
def test_attention_pooled_row_equals_full_attention(hd, L, causal):
    """clipx_attention_pooled_fwd / _bwd (one query row per sequence: the last block of a tower that is read at the pooled
    position) against the full attention kernels followed by the row gather / preceded by the row scatter, and against the
    fp32 reference: the class-token row of a vision tower (row 0, every key) and a random EOT row of a causal text tower
    (keys up to it; the rows behind it get exactly zero gradients)."""
    batch, heads = 5, 3
    d = heads * hd
    qkv = rnd(batch * L, 3 * d, seed=1, scale=2.0, dtype=torch.bfloat16)
    dout_s = rnd(batch, d, seed=2, dtype=torch.bfloat16)
    g = torch.Generator().manual_seed(L)
    pos = torch.randint(0, L, (batch,), generator=g) if causal else torch.zeros(batch, dtype=torch.long)
    if causal:
        pos[0], pos[1] = 0, L - 1
    idx = (torch.arange(batch) * L + pos).to(torch.int32).to(DEV)
    assert ops.attention_pooled_supported(torch.bfloat16, L, hd)
    o_s, lse = ops.attention_pooled_fwd(qkv, idx, batch, L, heads, causal)
    dq_s = ops.attention_pooled_bwd(qkv, dout_s, lse, idx, batch, L, heads, causal)
    # the same through the full kernels
    o_full = ops.attention_fwd(qkv, batch, L, heads, causal)
    do_full = ops.scatter_rows(dout_s, idx, batch * L)
    dq_full = ops.attention_bwd(qkv, do_full, batch, L, heads, causal)
    assert relerr(o_s, ops.gather_rows(o_full, idx)) < 1e-2
    assert relerr(dq_s, dq_full) < 1.5e-2
    # fp32 reference
    qf = qkv.float().detach().clone().requires_grad_(True)
    o_ref = attn_ref(qf, batch, L, heads, causal)
    o_ref.backward(do_full.float())
    assert relerr(o_s, o_ref[idx.long()]) < 1e-2
    assert relerr(dq_s, qf.grad) < 1.5e-2
    assert torch.isfinite(dq_s.float()).all()
    dq3 = dq_s.view(batch, L, 3, d)
    for s_ in range(batch):
        other = torch.ones(L, dtype=torch.bool)
        other[int(pos[s_])] = False
        assert float(dq3[s_, other.to(DEV), 0].float().abs().max()) == 0.0            # every other query row: exactly zero
        if causal and int(pos[s_]) + 1 < L:
            assert float(dq3[s_, int(pos[s_]) + 1:].float().abs().max()) == 0.0        # keys behind the pooled row: zero
    assert not ops.attention_pooled_supported(torch.bfloat16, 641, 64) and not ops.attention_pooled_supported(torch.float32, 50, 64)


def test_attention_pooled_row_on_packed_text():
    """The same on a TextLayout's packed rows (causal, the EOT row of every caption = its last packed row): equals the packed
    attention kernels on the live rows; the filler rows behind them get exactly zero."""
    batch, L, heads, hd, vocab = 300, 77, 2, 64, 500
    d = heads * hd
    text, lens = _captions(batch, L, vocab, seed=11)
    lay = ops.TextLayout(text.to(DEV), vocab)
    qkv = rnd(lay.rows, 3 * d, seed=1, scale=2.0, dtype=torch.bfloat16)
    dout_s = rnd(batch, d, seed=2, dtype=torch.bfloat16)
    o_s, lse = ops.attention_pooled_fwd(qkv, lay.eot_rows, batch, L, heads, True, lay)
    dq_s = ops.attention_pooled_bwd(qkv, dout_s, lse, lay.eot_rows, batch, L, heads, True, lay)
    o_full = ops.attention_packed_fwd(qkv, lay, heads, True)
    do_full = ops.scatter_rows(dout_s, lay.eot_rows, lay.rows)
    dq_full = ops.attention_packed_bwd(qkv, do_full, lay, heads, True)
    assert relerr(o_s, ops.gather_rows(o_full, lay.eot_rows)) < 1e-2
    assert relerr(dq_s[:lay.rows_live], dq_full[:lay.rows_live]) < 1.5e-2
    assert float(dq_s[lay.rows_live:].float().abs().max()) == 0.0


# ------------------------------------------------------------------ normalize / CE / params
def test_l2norm():
    x = rnd(33, 512, seed=1).requires_grad_(True)
    dy = rnd(33, 512, seed=2)
    ref = torch.nn.functional.normalize(x, dim=-1)
    ref.backward(dy)
    y, inv = ops.l2norm_fwd(x.detach())
    assert relerr(y, ref) < 1e-6
    assert relerr(ops.l2norm_bwd(dy, y, inv), x.grad) < 1e-5


@pytest.mark.parametrize("np_,nq,E,off,sym", [(50, 50, 64, 0, True), (6, 24, 16, 12, False), (200, 200, 512, 0, True),
                                              (130, 1000, 32, 300, False), (257, 257, 768, 0, True), (64, 4096, 1024, 1024, False),
                                              (100, 100, 128, 0, True), (70, 210, 256, 140, False), (300, 300, 640, 0, True)])
def test_fused_contrastive_ce(np_, nq, E, off, sym):
    """csrc/loss_fused.hip: loss, both log-sum-exps and every gradient of the contrastive cross-entropy without the logits
    matrix in memory, against plain fp32 PyTorch (reference loss.py:145-152,175-180 arithmetic)."""
    import torch.nn.functional as F
    a = F.normalize(rnd(np_, E, seed=1), dim=-1)
    b = F.normalize(rnd(nq, E, seed=2), dim=-1)
    scale = torch.tensor([17.3], device=DEV)
    w = 0.5 / np_
    ar, br, sr = a.clone().requires_grad_(True), b.clone().requires_grad_(True), scale.clone().requires_grad_(True)
    z = (sr * ar) @ br.t()
    lab = torch.arange(np_, device=DEV) + off
    ref = w * F.cross_entropy(z, lab, reduction="sum")
    if sym:
        ref = ref + w * F.cross_entropy(z.t(), torch.arange(nq, device=DEV), reduction="sum")
    gout = torch.tensor([0.7], device=DEV)
    (ref * gout[0]).backward()
    a_s = ops.scale_by_dev(a, scale)
    loss = torch.zeros(1, device=DEV)
    lse_r, lse_c = ops.ce_fused_fwd(a_s, b, off, sym, w, w, loss)
    assert abs(float(loss) - float(ref)) < 1e-5 * max(1.0, abs(float(ref)))
    assert relerr(lse_r, torch.logsumexp(z, 1)) < 1e-6
    if sym:
        assert relerr(lse_c, torch.logsumexp(z, 0)) < 1e-6
    dscale = torch.zeros(1, device=DEV)
    da = ops.ce_fused_bwd(a_s, b, lse_r, w, off, lse_c, w, 0, scale, gout, dscale, scale)
    db = ops.ce_fused_bwd(b, a_s, lse_c, w, 0, lse_r, w, off, None, gout)
    assert relerr(da, ar.grad) < 2e-5 and relerr(db, br.grad) < 2e-5
    assert abs(float(dscale * gout) - float(sr.grad)) < 2e-5 * max(1.0, abs(float(sr.grad)))


@pytest.mark.parametrize("rows,cols,off", [(16, 16, 0), (50, 200, 100), (130, 130, 0)])
def test_ce_kernels(rows, cols, off):
    z = rnd(rows, cols, seed=1, scale=4.0)
    lse = torch.empty(rows, device=DEV)
    loss = torch.zeros(1, device=DEV)
    ops.ce_rows(z, off, lse, 0.5 / rows, loss)
    labels = torch.arange(rows, device=DEV) + off
    ref = 0.5 * torch.nn.functional.cross_entropy(z, labels)
    assert relerr(lse, torch.logsumexp(z, -1)) < 1e-6
    assert abs(float(loss) - float(ref)) < 1e-5 * max(1.0, abs(float(ref)))
    lse_c = None
    if rows == cols:
        lse_c = torch.empty(cols, device=DEV)
        ops.ce_cols(z, lse_c, 0.5 / rows, loss)
        ref = ref + 0.5 * torch.nn.functional.cross_entropy(z.t(), labels)
        assert relerr(lse_c, torch.logsumexp(z, 0)) < 1e-6
        assert abs(float(loss) - float(ref)) < 1e-5 * max(1.0, abs(float(ref)))
    zf = z.clone().requires_grad_(True)
    l = 0.5 * torch.nn.functional.cross_entropy(zf, labels)
    if rows == cols:
        l = l + 0.5 * torch.nn.functional.cross_entropy(zf.t(), labels)
    l.backward()
    scale = torch.tensor([7.0], device=DEV)
    ds = torch.zeros(1, device=DEV)
    dz = z.clone()
    ops.ce_grad(dz, off, lse, 0.5 / rows, lse_c, 0.5 / rows, scale, ds)
    assert relerr(dz, zf.grad) < 1e-5
    assert abs(float(ds) - float((zf.grad * z).sum() / 7.0)) < 1e-5


def test_cast_weight_and_adamw():
    w = rnd(100, 72, seed=1)
    w16 = torch.empty(100, 72, dtype=torch.bfloat16, device=DEV)
    wt16 = torch.empty(72, 100, dtype=torch.bfloat16, device=DEV)
    ops.cast_weight(w, w16, wt16)
    assert torch.equal(w16, w.to(torch.bfloat16))
    assert torch.equal(wt16, w.to(torch.bfloat16).t().contiguous())
    for n in (1003, 4096):
        p = rnd(n, seed=2)
        ref_p = torch.nn.Parameter(p.clone())
        opt = torch.optim.AdamW([ref_p], lr=5e-4, betas=(0.9, 0.98), eps=1e-6, weight_decay=0.2)
        m, v = torch.zeros_like(p), torch.zeros_like(p)
        for step in range(1, 4):
            g = rnd(n, seed=10 + step)
            ref_p.grad = g.clone()
            opt.step()
            ops.adamw(p, g, m, v, 5e-4, 0.9, 0.98, 1e-6, 0.2, step)
            assert relerr(p, ref_p.detach()) < 1e-6
    acc = torch.zeros(1, device=DEV)
    ops.sumsq(p, acc)
    assert abs(float(acc) - float((p * p).sum())) < 1e-3 * float((p * p).sum())
    s = torch.tensor([5.0], device=DEV)
    ops.clamp1(s, 0.0, math.log(100))
    assert abs(float(s) - math.log(100)) < 1e-6


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("act", [ACT_GELU, ACT_QUICKGELU])
def test_act_bwd_colsum(dtype, act):
    M, N = 1003, 768
    dh = rnd(M, N, seed=1, dtype=dtype)
    u = rnd(M, N, seed=2, dtype=dtype)
    uf = u.float().detach().clone().requires_grad_(True)
    act_ref(act, uf).backward(dh.float())
    ws = torch.empty(ops.colsum_ws_bytes(M, N), dtype=torch.uint8, device=DEV)
    cs = torch.ones(N, device=DEV)
    du = ops.act_bwd_colsum(dh.clone(), u, act, cs, 1.0, ws)
    assert relerr(du, uf.grad) < (1e-5 if dtype == torch.float32 else 1e-2)
    # the kernel sums the fp32 products, the check sums the rounded outputs
    assert relerr(cs, uf.grad.sum(0) + 1.0) < (1e-4 if dtype == torch.float32 else 5e-3)


@pytest.mark.parametrize("M,N,K", [(512, 256, 128), (1000, 520, 192), (4096, 3072, 768), (300, 1024, 256)])
def test_linear_gelu_with_8bit_derivative(M, N, K):
    """The MLP's GELU with GELU'(pre-activation) kept on eight bits (csrc/gemm_epi.h G8_*, clipx_linear_fwd_gelu8 /
    clipx_linear_dgrad_gelu8; whole 256x256 tiles go through the wave-transposed 16-byte tile path, the edges through the
    per-quad path): y equals the bf16-pre-activation form bit for bit; the stored byte decodes to GELU'(u) of the UNROUNDED
    pre-activation within half a quantisation step (+ the polynomial's 2.7e-4); the dgrad equals (dy . W) * decoded factor to
    bf16 rounding; and against the exact erf derivative the factor is as close as the bf16 form's (which evaluates GELU' at a
    bf16-rounded u and rounds the product once more)."""
    dt = torch.bfloat16
    x = rnd(M, K, seed=1, dtype=dt)
    w = rnd(N, K, seed=2, scale=2.0 * K ** -0.5, dtype=dt)          # pre-activations over a few units: both tails of GELU'
    bias = rnd(N, seed=3)
    h_ref, u16 = ops.linear_fwd(x, w, bias, act=ACT_GELU, want_preact=True)
    h, g8 = ops.linear_fwd(x, w, bias, act=ACT_GELU, want_preact="gelu8")
    assert g8.dtype == torch.uint8 and g8.shape == (M, N)
    assert torch.equal(h, h_ref)
    u = x.double() @ w.double().t() + bias.double()
    exact = 0.5 * (1 + torch.erf(u / math.sqrt(2))) + u * torch.exp(-u * u / 2) / math.sqrt(2 * math.pi)
    lo, step = -0.13, 0.005
    dec = lo + step * g8.double()
    err = (dec - exact).abs()
    assert float(err.max()) < 0.5 * step + 6e-4, float(err.max())            # half a step + polynomial + fp32 accumulation of u
    # the dgrad: dx[M,N] = (dy[M,K2] . wt[N,K2]^T) * factor
    K2 = 256
    dy = rnd(M, K2, seed=4, dtype=dt)
    wt = rnd(N, K2, seed=5, scale=K2 ** -0.5, dtype=dt)
    dx = ops.linear_dgrad(dy, None, wt, act=ACT_GELU, u=g8)
    want = (dy.double() @ wt.double().t()) * dec
    assert relerr(dx, want.float()) < tol(dt)
    rel8 = float(((dx.double() - (dy.double() @ wt.double().t()) * exact).norm()) / ((dy.double() @ wt.double().t()) * exact).norm())
    dx16 = ops.linear_dgrad(dy, None, wt, act=ACT_GELU, u=u16)
    rel16 = float(((dx16.double() - (dy.double() @ wt.double().t()) * exact).norm()) / ((dy.double() @ wt.double().t()) * exact).norm())
    print(f"[gelu8 {M}x{N}x{K}] max |factor err| {float(err.max()):.2e} (step/2 = {0.5 * step:.2e}); dgrad vs exact erf derivative: "
          f"8-bit factor {rel8:.3e}, bf16 pre-activation {rel16:.3e}")
    assert rel8 < 1.5 * rel16 + 1e-3
