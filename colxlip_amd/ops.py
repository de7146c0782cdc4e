"""Tensor-level wrappers over the C ABI (include/clipx.h).

PyTorch is used only to own device memory and streams: every wrapper passes raw device
pointers of torch tensors plus the current HIP stream to libclipx_hip.so.  No wrapper
has a CPU or eager fallback; CPU tensors are rejected.
"""
import os
from typing import Optional

import torch

from . import _lib
from .trace import family
from ._lib import ACT_GELU, ACT_NONE, ACT_QUICKGELU, BF16, F32, check  # noqa: F401


def dt_code(dtype: torch.dtype) -> int:
    if dtype == torch.float32:
        return F32
    if dtype == torch.bfloat16:
        return BF16
    raise TypeError(f"unsupported dtype {dtype}")


def _p(t: Optional[torch.Tensor]):
    if t is None:
        return None
    if not t.is_cuda:
        raise RuntimeError("colxlip_amd ops need device (HIP) tensors; there is no CPU path")
    return t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _nt_stream():
    return _stream()


def _c(t: torch.Tensor) -> torch.Tensor:
    assert t.is_contiguous(), "clipx ops take contiguous tensors"
    return t


# ------------------------------------------------------------------ linear
@family("gemm_nt.fwd")
def linear_fwd(x, w, bias=None, act=ACT_NONE, want_preact=False, residual=None, out_dtype=None, out=None):
    """y = act(x @ w.T + bias) (+ residual).  x [M,K], w [N,K] in x.dtype; bias fp32."""
    M, K = x.shape
    N = w.shape[0]
    assert w.shape[1] == K and w.dtype == x.dtype
    out_dtype = out_dtype or (out.dtype if out is not None else x.dtype)
    y = out if out is not None else torch.empty((M, N), dtype=out_dtype, device=x.device)
    assert y.is_contiguous() and y.numel() == M * N and y.dtype == out_dtype
    if want_preact == "gelu8":
        # bf16 + GELU only: the epilogue keeps GELU'(x @ w.T + bias) on eight bits instead of the bf16 pre-activation
        # (csrc/gemm_epi.h, G8_*); linear_dgrad(u=<that uint8 tensor>) multiplies by it
        assert x.dtype == torch.bfloat16 and act == ACT_GELU and residual is None and out_dtype == torch.bfloat16
        g8 = torch.empty((M, N), dtype=torch.uint8, device=x.device)
        check(_lib.lib().clipx_linear_fwd_gelu8(M, N, K, _p(_c(x)), _p(_c(w)), _p(bias), _p(g8), _p(y), _nt_stream()))
        return y, g8
    u = torch.empty((M, N), dtype=x.dtype, device=x.device) if want_preact else None
    check(_lib.lib().clipx_linear_fwd(dt_code(x.dtype), M, N, K, _p(_c(x)), _p(_c(w)), _p(bias), act, _p(u),
                                      _p(residual), _p(y), dt_code(out_dtype), _nt_stream()))
    return (y, u) if want_preact else y


def quant_rows_e4m3(x):
    """x [M,K] bf16 -> (x8 [M,K] uint8 of e4m3 bytes, row_exp [M] int32): the activation operand of linear_fwd_fp8."""
    M, K = x.shape
    assert x.dtype == torch.bfloat16
    x8 = torch.empty((M, K), dtype=torch.uint8, device=x.device)
    xe = torch.empty((M,), dtype=torch.int32, device=x.device)
    check(_lib.lib().clipx_quant_rows_e4m3(M, K, _p(_c(x)), _p(xe), _p(x8), _stream()))
    return x8, xe


def quant_tokens_e4m3(tokens):
    """tokens [n, q, E] bf16 -> (bytes [n, q, E] uint8 of e4m3, exp [n, q] int32): `quant_rows_e4m3` on the n * q token rows, one
    power-of-two exponent per token.  The stored form of a late-interaction index (search.py) and the operand form of
    `maxsim_scores_fp8`."""
    n, q, e = tokens.shape
    assert tokens.dtype == torch.bfloat16
    if n * q == 0:
        return (torch.empty((n, q, e), dtype=torch.uint8, device=tokens.device),
                torch.empty((n, q), dtype=torch.int32, device=tokens.device))
    x8, xe = quant_rows_e4m3(tokens.contiguous().view(n * q, e))
    return x8.view(n, q, e), xe.view(n, q)


def dequant_tokens_e4m3(x8, exp, dtype=torch.float32):
    """(bytes [..., E] uint8, exp [...] int32) -> bytes read as float8_e4m3fn times 2^exp, in `dtype`; plain torch, CPU tensors too.
    Every value is exact in fp32 and in bf16 (three mantissa bits)."""
    assert x8.dtype == torch.uint8 and x8.shape[:-1] == exp.shape
    return torch.ldexp(x8.view(torch.float8_e4m3fn).to(torch.float32), exp.unsqueeze(-1).to(torch.int32)).to(dtype)


@family("gemm_nt.fwd_fp8")
def linear_fwd_fp8(x8, xe, w8, we, bias=None, act=ACT_NONE, want_preact=False, residual=None, out=None):
    """y (bf16) = act(2^(xe[m] + we[n]) * x8 @ w8.T + bias) (+ residual) on the fp8 MFMA.  x8 [M,K], w8 [N,K] uint8 (e4m3)."""
    M, K = x8.shape
    N = w8.shape[0]
    assert w8.shape[1] == K and x8.dtype == torch.uint8 and w8.dtype == torch.uint8
    y = out if out is not None else torch.empty((M, N), dtype=torch.bfloat16, device=x8.device)
    if want_preact == "gelu8":
        assert act == ACT_GELU and residual is None
        g8 = torch.empty((M, N), dtype=torch.uint8, device=x8.device)
        check(_lib.lib().clipx_linear_fwd_fp8_gelu8(M, N, K, _p(_c(x8)), _p(xe), _p(_c(w8)), _p(we), _p(bias), _p(g8), _p(y), _stream()))
        return y, g8
    u = torch.empty((M, N), dtype=torch.bfloat16, device=x8.device) if want_preact else None
    check(_lib.lib().clipx_linear_fwd_fp8(M, N, K, _p(_c(x8)), _p(xe), _p(_c(w8)), _p(we), _p(bias), act, _p(u), _p(residual),
                                          _p(y), _stream()))
    return (y, u) if want_preact else y


@family("gemm_nt.dgrad_fp8")
def linear_dgrad_fp8(dy8, dye, wt8, wte, act=ACT_NONE, u=None, out=None):
    """dx (bf16) [M,K] = 2^(dye[m] + wte[k]) * dy8 [M,N] @ wt8 [K,N].T (optionally * act'(u)) on the fp8 MFMA."""
    M, N = dy8.shape
    K = wt8.shape[0]
    assert wt8.shape[1] == N and dy8.dtype == torch.uint8 and wt8.dtype == torch.uint8
    dx = out if out is not None else torch.empty((M, K), dtype=torch.bfloat16, device=dy8.device)
    if u is not None and u.dtype == torch.uint8:
        assert act == ACT_GELU and u.shape == (M, K) and u.is_contiguous()
        check(_lib.lib().clipx_linear_dgrad_fp8_gelu8(M, N, K, _p(_c(dy8)), _p(dye), _p(_c(wt8)), _p(wte), _p(u), _p(dx), _stream()))
        return dx
    check(_lib.lib().clipx_linear_dgrad_fp8(M, N, K, _p(_c(dy8)), _p(dye), _p(_c(wt8)), _p(wte), act, _p(u), _p(dx), _stream()))
    return dx


@family("gemm_nt.dgrad")
def linear_dgrad(dy, w, wt, act=ACT_NONE, u=None, out=None):
    """dx = dy @ w (optionally * act'(u)).  w [N,K] (fp32 mode) / wt [K,N] (bf16 mode)."""
    M, N = dy.shape
    K = w.shape[1] if w is not None else wt.shape[0]
    dx = out if out is not None else torch.empty((M, K), dtype=dy.dtype, device=dy.device)
    if u is not None and u.dtype == torch.uint8:      # the 8-bit GELU' factor written by linear_fwd(want_preact="gelu8")
        assert dy.dtype == torch.bfloat16 and act == ACT_GELU and u.shape == (M, K) and u.is_contiguous()
        check(_lib.lib().clipx_linear_dgrad_gelu8(M, N, K, _p(_c(dy)), _p(wt), _p(u), _p(dx), _nt_stream()))
        return dx
    check(_lib.lib().clipx_linear_dgrad(dt_code(dy.dtype), M, N, K, _p(_c(dy)), _p(w), _p(wt), act, _p(u), _p(dx),
                                        _nt_stream()))
    return dx


@family("gemm_tn.wgrad")
def linear_wgrad(dy, x, dw, beta, ws, db=None, beta_b=0.0):
    """dw[N,K] (fp32) = beta*dw + dy.T @ x; with db also db[N] = beta_b*db + dy.sum(0) from the same pass."""
    M, N = dy.shape
    K = x.shape[1]
    assert dw.dtype == torch.float32 and dw.is_contiguous() and dw.numel() == N * K
    assert db is None or (db.dtype == torch.float32 and db.is_contiguous() and db.numel() == N)
    check(_lib.lib().clipx_linear_wgrad(dt_code(dy.dtype), M, N, K, _p(_c(dy)), _p(_c(x)), _p(dw), float(beta),
                                        _p(db), float(beta_b), _p(ws),
                                        ws.numel() * ws.element_size() if ws is not None else 0, _stream()))


def linear_wgrad_ws_bytes(dtype, M, N, K) -> int:
    return int(_lib.lib().clipx_linear_wgrad_ws_bytes(dt_code(dtype), M, N, K))


def _c_arrays(problems):
    """ctypes host arrays for clipx_linear_wgrad_group from [(dy, x, dw, beta, db, beta_b), ...]."""
    import ctypes
    n = len(problems)
    IntA, PtrA, FltA = ctypes.c_int * n, ctypes.c_void_p * n, ctypes.c_float * n
    N = IntA(*[p[0].shape[1] for p in problems])
    K = IntA(*[p[1].shape[1] for p in problems])
    dy = PtrA(*[p[0].data_ptr() for p in problems])
    x = PtrA(*[p[1].data_ptr() for p in problems])
    dw = PtrA(*[p[2].data_ptr() for p in problems])
    beta = FltA(*[float(p[3]) for p in problems])
    db = PtrA(*[(p[4].data_ptr() if p[4] is not None else None) for p in problems])
    beta_b = FltA(*[float(p[5]) for p in problems])
    return N, K, dy, x, dw, beta, db, beta_b


def linear_wgrad_group_ws_bytes(dtype, M, shapes) -> int:
    """Workspace bytes for linear_wgrad_group over [(N, K), ...]."""
    import ctypes
    n = len(shapes)
    N = (ctypes.c_int * n)(*[s[0] for s in shapes])
    K = (ctypes.c_int * n)(*[s[1] for s in shapes])
    return int(_lib.lib().clipx_linear_wgrad_group_ws_bytes(dt_code(dtype), M, n, N, K))


@family("gemm_tn.wgrad")
def linear_wgrad_group(problems, ws):
    """Up to four wgrads over the same M rows as ONE launch: problems = [(dy [M,N], x [M,K], dw [N,K] fp32, beta, db or None,
    beta_b), ...] (include/clipx.h, clipx_linear_wgrad_group)."""
    M = problems[0][0].shape[0]
    dt = problems[0][0].dtype
    keep = []
    for dy, x, dw, beta, db, beta_b in problems:
        assert dy.shape[0] == M and x.shape[0] == M and dy.dtype == dt and x.dtype == dt
        assert dy.is_contiguous() and x.is_contiguous()
        assert dw.dtype == torch.float32 and dw.is_contiguous() and dw.numel() == dy.shape[1] * x.shape[1]
        assert db is None or (db.dtype == torch.float32 and db.is_contiguous() and db.numel() == dy.shape[1])
    N, K, dyp, xp, dwp, beta, dbp, beta_b = _c_arrays(problems)
    check(_lib.lib().clipx_linear_wgrad_group(dt_code(dt), M, len(problems), N, K, dyp, xp, dwp, beta, dbp, beta_b, _p(ws),
                                              ws.numel() * ws.element_size(), _stream()))


def colsum(a, out, beta, ws):
    M, N = a.shape
    check(_lib.lib().clipx_colsum(dt_code(a.dtype), M, N, _p(_c(a)), _p(out), float(beta), _p(ws),
                                  ws.numel() * ws.element_size(), _stream()))


def act_bwd_colsum(dh, u, act, colsum_out, beta, ws, out=None):
    """du = dh * act'(u) (written to `out`, default in place over dh) and colsum_out = beta*colsum_out + du.sum(0)."""
    M, N = dh.shape
    out = dh if out is None else out
    check(_lib.lib().clipx_act_bwd_colsum(dt_code(dh.dtype), M, N, act, _p(_c(dh)), _p(_c(u)), _p(out), _p(colsum_out),
                                          float(beta), _p(ws), ws.numel() * ws.element_size(), _stream()))
    return out


def colsum_ws_bytes(M, N) -> int:
    return int(_lib.lib().clipx_colsum_ws_bytes(M, N))


@family("gemm_f32")
def gemm_f32(M, N, K, A, a_rs, a_cs, B, b_rs, b_cs, C, ldc, alpha=1.0, beta=0.0):
    assert A.dtype == B.dtype == C.dtype == torch.float32
    check(_lib.lib().clipx_gemm_f32(M, N, K, _p(A), a_rs, a_cs, _p(B), b_rs, b_cs, _p(C), ldc, float(alpha),
                                    float(beta), _stream()))


# ------------------------------------------------------------------ layernorm
@family("layernorm.fwd")
def layernorm_fwd(x, gamma, beta, rows=None, row_index=None, eps=1e-5, out=None):
    width = x.shape[-1]
    rows = rows if rows is not None else x.numel() // width
    y = out if out is not None else torch.empty((rows, width), dtype=x.dtype, device=x.device)
    assert y.is_contiguous() and y.shape[0] == rows and y.dtype == x.dtype
    mean = torch.empty((rows,), dtype=torch.float32, device=x.device)
    rstd = torch.empty((rows,), dtype=torch.float32, device=x.device)
    check(_lib.lib().clipx_layernorm_fwd(dt_code(x.dtype), rows, width, _p(_c(x)), _p(row_index), _p(gamma), _p(beta),
                                         float(eps), _p(y), _p(mean), _p(rstd), _stream()))
    return y, mean, rstd


def layernorm_fwd_q8(x, gamma, beta, eps=1e-5):
    """LayerNorm forward of a bf16 [rows, width] tensor that also returns the rows in the fp8 MFMA linear's operand form:
    (y, mean, rstd, y8 uint8 [rows, width], y_exp int32 [rows]) -- y8 / y_exp equal quant_rows_e4m3(y) bit for bit."""
    rows, width = x.shape
    assert x.dtype == torch.bfloat16
    y = torch.empty((rows, width), dtype=x.dtype, device=x.device)
    y8 = torch.empty((rows, width), dtype=torch.uint8, device=x.device)
    ye = torch.empty((rows,), dtype=torch.int32, device=x.device)
    mean = torch.empty((rows,), dtype=torch.float32, device=x.device)
    rstd = torch.empty((rows,), dtype=torch.float32, device=x.device)
    check(_lib.lib().clipx_layernorm_fwd_q8(rows, width, _p(_c(x)), _p(gamma), _p(beta), float(eps), _p(y), _p(mean), _p(rstd),
                                            _p(y8), _p(ye), _stream()))
    return y, mean, rstd, y8, ye


def layernorm_ws_bytes(width) -> int:
    return int(_lib.lib().clipx_layernorm_ws_bytes(width))


@family("layernorm.bwd")
def layernorm_bwd(dy, x, gamma, mean, rstd, ws, dx_res=None, dx_out=None, row_index=None):
    """Returns dx_out; leaves (dgamma, dbeta, colsum(dx_out)) partials in ws for layernorm_bwd_finish."""
    rows, width = dy.shape
    if dx_out is None:
        dx_out = torch.empty_like(x)
    check(_lib.lib().clipx_layernorm_bwd(dt_code(dy.dtype), rows, width, _p(_c(dy)), _p(_c(x)), _p(row_index),
                                         _p(gamma), _p(mean), _p(rstd), _p(dx_res), _p(dx_out), _p(ws),
                                         ws.numel() * ws.element_size(), _stream()))
    return dx_out


@family("layernorm.bwd")
def layernorm_bwd_finish(width, ws, dgamma, dbeta, colsum_out, beta):
    check(_lib.lib().clipx_layernorm_bwd_finish(width, _p(ws), _p(dgamma), _p(dbeta), _p(colsum_out), float(beta),
                                                _stream()))


# ------------------------------------------------------------------ attention
@family("attention.fwd")
def attention_fwd(qkv, batch, L, heads, causal, want_lse=False):
    """out [batch*L, d]; with want_lse also the log-sum-exp [batch*heads, L] (None for shapes without that hand-over:
    clipx_attention_lse_supported) -- pass both to attention_bwd."""
    d3 = qkv.shape[-1]
    d = d3 // 3
    out = torch.empty((batch * L, d), dtype=qkv.dtype, device=qkv.device)
    if want_lse and batch > 0 and _lib.lib().clipx_attention_lse_supported(dt_code(qkv.dtype), L, d // heads):
        lse = torch.empty((batch * heads, L), dtype=torch.float32, device=qkv.device)
        check(_lib.lib().clipx_attention_fwd_lse(dt_code(qkv.dtype), batch, L, heads, d // heads, int(causal), _p(_c(qkv)),
                                                 _p(out), _p(lse), _stream()))
        return out, lse
    check(_lib.lib().clipx_attention_fwd(dt_code(qkv.dtype), batch, L, heads, d // heads, int(causal), _p(_c(qkv)),
                                         _p(out), _stream()))
    return (out, None) if want_lse else out


@family("attention.bwd")
def attention_bwd(qkv, dout, batch, L, heads, causal, out=None, lse=None):
    """dqkv; `out` + `lse` (attention_fwd(..., want_lse=True)) let the online-softmax kernels skip their statistics sweep."""
    d = qkv.shape[-1] // 3
    dqkv = torch.empty_like(qkv)
    if lse is not None and out is not None:
        check(_lib.lib().clipx_attention_bwd_lse(dt_code(qkv.dtype), batch, L, heads, d // heads, int(causal), _p(_c(qkv)),
                                                 _p(_c(dout)), _p(_c(out)), _p(lse), _p(dqkv), _stream()))
        return dqkv
    check(_lib.lib().clipx_attention_bwd(dt_code(qkv.dtype), batch, L, heads, d // heads, int(causal), _p(_c(qkv)),
                                         _p(_c(dout)), _p(dqkv), _stream()))
    return dqkv


@family("attention.fwd")
def attention_packed_fwd(qkv, layout, heads, causal):
    """Attention over packed rows (TextLayout): one launch per non-empty length bucket."""
    d = qkv.shape[-1] // 3
    out = torch.empty((qkv.shape[0], d), dtype=qkv.dtype, device=qkv.device)
    L = _lib.lib()
    for first, count, max_len in layout.buckets:
        check(L.clipx_attention_packed_fwd(dt_code(qkv.dtype), count, max_len, heads, d // heads, int(causal),
                                           layout.order.data_ptr() + 4 * first, _p(layout.cu), _p(_c(qkv)), _p(out),
                                           _stream()))
    return out


@family("attention.bwd")
def attention_packed_bwd(qkv, dout, layout, heads, causal):
    d = qkv.shape[-1] // 3
    dqkv = torch.empty_like(qkv)
    L = _lib.lib()
    for first, count, max_len in layout.buckets:
        check(L.clipx_attention_packed_bwd(dt_code(qkv.dtype), count, max_len, heads, d // heads, int(causal),
                                           layout.order.data_ptr() + 4 * first, _p(layout.cu), _p(_c(qkv)),
                                           _p(_c(dout)), _p(dqkv), _stream()))
    return dqkv


def attention_pooled_supported(dtype, max_len, hd) -> bool:
    return bool(_lib.lib().clipx_attention_pooled_supported(dt_code(dtype), int(max_len), int(hd)))


@family("attention.fwd")
def attention_pooled_fwd(qkv, idx, batch, L, heads, causal, layout=None):
    """Attention output of the ONE query row idx[s] of every sequence: (out [batch, d], lse [batch*heads]).  Dense rows
    (sequence s = rows s*L ..) or a TextLayout's packed rows."""
    d = qkv.shape[-1] // 3
    out = torch.empty((batch, d), dtype=qkv.dtype, device=qkv.device)
    lse = torch.empty((batch * heads,), dtype=torch.float32, device=qkv.device)
    cu = _p(layout.cu) if layout is not None else None
    max_len = layout.longest if layout is not None else L
    check(_lib.lib().clipx_attention_pooled_fwd(dt_code(qkv.dtype), batch, 0 if layout is not None else L, max_len, heads, d // heads,
                                                int(causal), _p(_c(qkv)), _p(idx), cu, _p(out), _p(lse), _stream()))
    return out, lse


@family("attention.bwd")
def attention_pooled_bwd(qkv, dout, lse, idx, batch, L, heads, causal, layout=None):
    """dqkv [rows, 3d] from the gradient of the pooled rows' attention output (dout [batch, d])."""
    d = qkv.shape[-1] // 3
    dqkv = torch.empty_like(qkv)
    cu = _p(layout.cu) if layout is not None else None
    max_len = layout.longest if layout is not None else L
    if layout is not None and layout.rows > layout.rows_live:
        dqkv[layout.rows_live:].zero_()                       # the filler sequences behind the live rows: exactly zero gradient
    check(_lib.lib().clipx_attention_pooled_bwd(dt_code(qkv.dtype), batch, 0 if layout is not None else L, max_len, heads, d // heads,
                                                int(causal), _p(_c(qkv)), _p(_c(dout)), _p(lse), _p(idx), cu, _p(dqkv), _stream()))
    return dqkv


@family("attention.fwd")
def attention_pooled_fwd_split(q, kv, idx, batch, L, heads, causal, layout=None):
    """attention_pooled_fwd on a split in_proj: q [batch, d] (the pooled rows' queries), kv [rows, 2 d]."""
    d = q.shape[-1]
    out = torch.empty((batch, d), dtype=q.dtype, device=q.device)
    lse = torch.empty((batch * heads,), dtype=torch.float32, device=q.device)
    cu = _p(layout.cu) if layout is not None else None
    max_len = layout.longest if layout is not None else L
    check(_lib.lib().clipx_attention_pooled_fwd_split(dt_code(q.dtype), batch, 0 if layout is not None else L, max_len, heads,
                                                      d // heads, int(causal), _p(_c(q)), _p(_c(kv)), _p(idx), cu, _p(out), _p(lse),
                                                      _stream()))
    return out, lse


@family("attention.bwd")
def attention_pooled_bwd_split(q, kv, dout, lse, idx, batch, L, heads, causal, layout=None):
    """(dq [batch, d], dkv [rows, 2 d])."""
    d = q.shape[-1]
    dq = torch.empty_like(q)
    dkv = torch.empty_like(kv)
    cu = _p(layout.cu) if layout is not None else None
    max_len = layout.longest if layout is not None else L
    if layout is not None and layout.rows > layout.rows_live:
        dkv[layout.rows_live:].zero_()                        # the filler sequences behind the live rows: exactly zero gradient
    check(_lib.lib().clipx_attention_pooled_bwd_split(dt_code(q.dtype), batch, 0 if layout is not None else L, max_len, heads,
                                                      d // heads, int(causal), _p(_c(q)), _p(_c(kv)), _p(_c(dout)), _p(lse), _p(idx),
                                                      cu, _p(dq), _p(dkv), _stream()))
    return dq, dkv


# ------------------------------------------------------------------ embeddings
@family("embed")
def patchify(image, P, Kp, dtype):
    b, c, H, W = image.shape
    assert c == 3
    G2 = (H // P) * (W // P)
    out = torch.empty((b * G2, Kp), dtype=dtype, device=image.device)
    check(_lib.lib().clipx_patchify(dt_code(image.dtype), dt_code(dtype), b, H, W, P, Kp, _p(_c(image)), _p(out),
                                    _stream()))
    return out


IMAGE_MAX_SCALE = 16        # box / virtual output per axis: IT_MAX_SCALE of csrc/image_transform.hip


def image_geometry(offsets, hw, box, vsize, origin, out_hw, nbytes, allow_partial=False):
    """Validate the per-image geometry of `image_transform` on the host and pack it into the kernel's records: a CPU int64
    tensor [n, 6] (48 bytes per image: int64 offset, then int32 h, w, top, left, bh, bw, vh, vw, oy, ox).
    offsets [n] byte offset of each HWC uint8 image in a buffer of `nbytes`; hw [n, 2] its (h, w); box [n, 4] source box
    (top, left, bh, bw); vsize [n, 2] virtual output (vh, vw); origin [n, 2] origin (oy, ox) of the out_hw window in it.
    Raises ValueError -- before anything is launched -- for an image outside the buffer, a box outside its image, a window outside
    the virtual output, or a scale (box / virtual size) above IMAGE_MAX_SCALE on either axis.  allow_partial: a window may reach
    past the right / bottom edge of its virtual output; the kernel leaves that part of the output untouched."""
    H, W = int(out_hw[0]), int(out_hw[1])
    offsets = torch.as_tensor(offsets, dtype=torch.int64).reshape(-1)
    n = offsets.numel()
    geom = torch.cat([torch.as_tensor(t, dtype=torch.int64).reshape(n, k) for t, k in ((hw, 2), (box, 4), (vsize, 2), (origin, 2))],
                     dim=1)
    h, w, top, left, bh, bw, vh, vw, oy, ox = geom.unbind(1)
    if H < 1 or W < 1:
        raise ValueError(f"image_transform: output size {H} x {W}")
    if n and bool(((h < 1) | (w < 1) | (offsets < 0) | (offsets + 3 * h * w > int(nbytes))).any()):
        raise ValueError("image_transform: an image does not lie inside the byte buffer")
    if n and bool(((top < 0) | (left < 0) | (bh < 1) | (bw < 1) | (top + bh > h) | (left + bw > w)).any()):
        raise ValueError("image_transform: a source box does not lie inside its image")
    outside = ((oy >= vh) | (ox >= vw)) if allow_partial else ((oy + H > vh) | (ox + W > vw))
    if n and bool(((vh < 1) | (vw < 1) | (oy < 0) | (ox < 0) | outside).any()):
        raise ValueError("image_transform: the output window does not lie inside the virtual output")
    if n and bool(((bh > IMAGE_MAX_SCALE * vh) | (bw > IMAGE_MAX_SCALE * vw)).any()):
        raise ValueError(f"image_transform: a box is more than {IMAGE_MAX_SCALE}x its output size on an axis "
                         "(store smaller images: python -m colxlip_amd.pack --max-side)")
    meta = torch.empty((n, 6), dtype=torch.int64)
    meta[:, 0] = offsets
    meta.view(torch.int32)[:, 2:] = geom.to(torch.int32)
    return meta


@family("embed")
def image_transform(data, meta, out_hw, mean, std, interpolation="bicubic", dtype=torch.float32, out=None):
    """uint8 HWC images -> normalised [n, 3, H, W] `dtype` (fp32 | bf16): crop, PIL-exact two-pass resample (bicubic | bilinear),
    (level / 255 - mean) / std, in one kernel.  data: 1-D uint8 device buffer; meta: the records of `image_geometry` (a CPU tensor
    is copied to the device; a device tensor is used as it is and must come from `image_geometry`)."""
    if interpolation not in ("bicubic", "bilinear"):
        raise ValueError(f"image_transform: interpolation {interpolation!r} (bicubic | bilinear)")
    assert data.dtype == torch.uint8 and data.dim() == 1 and meta.dtype == torch.int64 and meta.dim() == 2 and meta.shape[1] == 6
    if not meta.is_cuda:
        meta = meta.to(data.device)
    n, (H, W) = meta.shape[0], (int(out_hw[0]), int(out_hw[1]))
    if out is None:
        out = torch.empty((n, 3, H, W), dtype=dtype, device=data.device)
    assert out.shape == (n, 3, H, W) and out.dtype == dtype
    m, s = [float(v) for v in mean], [float(v) for v in std]
    check(_lib.lib().clipx_image_transform(n, _p(_c(data)), data.numel(), _p(_c(meta)), H, W, m[0], m[1], m[2], s[0], s[1], s[2],
                                           1 if interpolation == "bicubic" else 0, dt_code(dtype), _p(_c(out)), _stream()))
    return out


@family("embed")
def vision_assemble(tok, cls, pos, batch, tokens):
    width = tok.shape[-1]
    x0 = torch.empty((batch * tokens, width), dtype=tok.dtype, device=tok.device)
    check(_lib.lib().clipx_vision_assemble(dt_code(tok.dtype), batch, tokens, width, _p(_c(tok)), _p(cls), _p(pos),
                                           _p(x0), _stream()))
    return x0


@family("embed")
def vision_assemble_bwd(dx0, batch, tokens, dpos, dcls, beta):
    width = dx0.shape[-1]
    dtok = torch.empty((batch * (tokens - 1), width), dtype=dx0.dtype, device=dx0.device)
    nbytes = int(_lib.lib().clipx_vision_assemble_bwd_ws_bytes(tokens, width))
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=dx0.device)
    check(_lib.lib().clipx_vision_assemble_bwd(dt_code(dx0.dtype), batch, tokens, width, _p(_c(dx0)), _p(dtok),
                                               _p(dpos), _p(dcls), float(beta), _p(ws), nbytes, _stream()))
    return dtok


@family("embed")
def patch_keep_index(batch, G2, keep, key, device):
    """int32 [batch, keep]: `keep` distinct patch positions of [0, G2) per sample, uniform, ascending; a function of the
    63-bit `key` and the sample index only (patch dropout's mask, drawn on the device)."""
    idx = torch.empty((batch, keep), dtype=torch.int32, device=device)
    check(_lib.lib().clipx_patch_keep_index(batch, G2, keep, int(key), _p(idx), _stream()))
    return idx


@family("embed")
def patchify_keep(image, P, Kp, dtype, keep_idx):
    """The rows of patchify(image, P, Kp, dtype) picked by keep_idx [b, keep]: [b*keep, Kp]."""
    b, c, H, W = image.shape
    assert c == 3 and keep_idx.dtype == torch.int32 and keep_idx.shape[0] == b
    keep = keep_idx.shape[1]
    out = torch.empty((b * keep, Kp), dtype=dtype, device=image.device)
    check(_lib.lib().clipx_patchify_keep(dt_code(image.dtype), dt_code(dtype), b, H, W, P, Kp, keep, _p(_c(keep_idx)),
                                         _p(_c(image)), _p(out), _stream()))
    return out


@family("embed")
def vision_assemble_keep(tok, cls, pos, keep_idx, G2):
    """x0 [b*(1+keep), width]: cls + pos[0], then tok[b*keep + j] + pos[1 + keep_idx[b, j]]."""
    batch, keep = keep_idx.shape
    width = tok.shape[-1]
    x0 = torch.empty((batch * (keep + 1), width), dtype=tok.dtype, device=tok.device)
    check(_lib.lib().clipx_vision_assemble_keep(dt_code(tok.dtype), batch, keep, G2, width, _p(_c(tok)), _p(cls), _p(pos),
                                                _p(_c(keep_idx)), _p(x0), _stream()))
    return x0


@family("embed")
def vision_assemble_keep_bwd(dx0, keep_idx, G2, dpos, dcls, beta):
    """dtok [b*keep, width]; dpos / dcls = beta * themselves + the gradient scattered to the kept positions."""
    batch, keep = keep_idx.shape
    width = dx0.shape[-1]
    dtok = torch.empty((batch * keep, width), dtype=dx0.dtype, device=dx0.device)
    nbytes = int(_lib.lib().clipx_vision_assemble_keep_bwd_ws_bytes(G2, width))
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=dx0.device)
    check(_lib.lib().clipx_vision_assemble_keep_bwd(dt_code(dx0.dtype), batch, keep, G2, width, _p(_c(dx0)), _p(_c(keep_idx)),
                                                    _p(dtok), _p(dpos), _p(dcls), float(beta), _p(ws), nbytes, _stream()))
    return dtok


@family("embed")
def text_embed(text, table, pos, dtype):
    b, L = text.shape
    vocab, width = table.shape
    assert text.dtype == torch.int64
    x0 = torch.empty((b * L, width), dtype=dtype, device=text.device)
    check(_lib.lib().clipx_text_embed(dt_code(dtype), b, L, width, vocab, _p(_c(text)), _p(table), _p(pos), _p(x0),
                                      _stream()))
    return x0


@family("embed")
def text_embed_bwd(text, dx0, dtable, dpos, beta):
    b, L = text.shape
    vocab, width = dtable.shape
    nbytes = int(_lib.lib().clipx_text_embed_bwd_ws_bytes(L, width, vocab))
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=dx0.device)
    check(_lib.lib().clipx_text_embed_bwd(dt_code(dx0.dtype), b, L, width, vocab, _p(_c(text)), _p(_c(dx0)),
                                          _p(dtable), _p(dpos), float(beta), _p(ws), nbytes, _stream()))


def gather_rows(src, row_index):
    rows, width = row_index.shape[0], src.shape[-1]
    dst = torch.empty((rows, width), dtype=src.dtype, device=src.device)
    check(_lib.lib().clipx_gather_rows(dt_code(src.dtype), rows, width, _p(_c(src)), _p(row_index), _p(dst), _stream()))
    return dst


def scatter_rows(src, row_index, dst_rows):
    """[dst_rows, width] zeros with dst[row_index[r]] = src[r]."""
    rows, width = src.shape
    dst = torch.empty((dst_rows, width), dtype=src.dtype, device=src.device)
    check(_lib.lib().clipx_scatter_rows(dt_code(src.dtype), dst_rows, rows, width, _p(_c(src)), _p(row_index), _p(dst), 0,
                                        _stream()))
    return dst


def scatter_add_rows(src, row_index, dst):
    rows, width = src.shape
    check(_lib.lib().clipx_scatter_rows(dt_code(src.dtype), dst.shape[0], rows, width, _p(_c(src)), _p(row_index), _p(_c(dst)),
                                        1, _stream()))
    return dst


class TextLayout:
    """Packed ("unpadded") row layout of a batch of captions, built on the device by clipx_text_layout: only positions
    0..EOT of each caption are kept (everything behind the EOT is dead under the causal mask + EOT pooling).  The host
    reads back eight integers (row count, sequence count, bucket sizes) -- the one synchronisation point of the path."""

    ROW_ALIGN = 256

    def __init__(self, text, vocab):
        b, L = text.shape
        assert text.dtype == torch.int64 and text.is_cuda
        dev = text.device
        self.batch, self.L = b, L
        self.header_dev = torch.empty((8,), dtype=torch.int32, device=dev)
        self.cu = torch.empty((b + 65,), dtype=torch.int32, device=dev)
        self.order = torch.empty((b + 64,), dtype=torch.int32, device=dev)
        self.row_tok = torch.empty((b * L + self.ROW_ALIGN,), dtype=torch.int32, device=dev)
        self.row_pos = torch.empty((b * L + self.ROW_ALIGN,), dtype=torch.int32, device=dev)
        check(_lib.lib().clipx_text_layout(b, L, vocab, self.ROW_ALIGN, _p(_c(text)), _p(self.header_dev), _p(self.cu),
                                           _p(self.order), _p(self.row_tok), _p(self.row_pos), _stream()))
        h = self.header_dev.cpu().tolist()                  # stream sync: the sizes below shape every later launch
        self.rows_live, self.rows, self.nseq = h[0], h[1], h[2]
        self.longest = h[6]
        self.buckets = []                                   # (first index into order[], count, max_len of the bucket)
        first = 0
        for count, cap in zip(h[3:6], (32, 64, max(h[6], 65))):
            if count > 0:
                self.buckets.append((first, count, min(cap, max(h[6], 1))))
            first += count
        self.eot_rows = torch.empty((b,), dtype=torch.int32, device=dev)
        check(_lib.lib().clipx_packed_eot_index(b, _p(self.cu), _p(self.eot_rows), _stream()))


@family("embed")
def text_embed_packed(layout, table, pos, dtype):
    vocab, width = table.shape
    x0 = torch.empty((layout.rows, width), dtype=dtype, device=table.device)
    check(_lib.lib().clipx_text_embed_packed(dt_code(dtype), layout.rows, width, _p(layout.row_tok), _p(layout.row_pos),
                                             _p(table), _p(pos), _p(x0), _stream()))
    return x0


@family("embed")
def text_embed_packed_bwd(layout, dx0, dtable, dpos, beta):
    vocab, width = dtable.shape
    nbytes = int(_lib.lib().clipx_text_embed_packed_bwd_ws_bytes(layout.L, width, vocab))
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=dx0.device)
    check(_lib.lib().clipx_text_embed_packed_bwd(dt_code(dx0.dtype), layout.rows, layout.nseq, layout.L, width, vocab,
                                                 _p(layout.row_tok), _p(layout.cu), _p(_c(dx0)), _p(dtable), _p(dpos),
                                                 float(beta), _p(ws), nbytes, _stream()))


def eot_index(text):
    b, L = text.shape
    idx = torch.empty((b,), dtype=torch.int32, device=text.device)
    check(_lib.lib().clipx_eot_index(b, L, _p(_c(text)), _p(idx), _stream()))
    return idx


def stride_index(batch, stride, device):
    idx = torch.empty((batch,), dtype=torch.int32, device=device)
    check(_lib.lib().clipx_stride_index(batch, stride, _p(idx), _stream()))
    return idx


# ------------------------------------------------------------------ normalize / loss pieces
def l2norm_fwd(x):
    rows, width = x.shape
    y = torch.empty_like(x)
    inv = torch.empty((rows,), dtype=torch.float32, device=x.device)
    check(_lib.lib().clipx_l2norm_fwd(rows, width, _p(_c(x)), _p(y), _p(inv), _stream()))
    return y, inv


def l2norm_bwd(dy, y, inv):
    rows, width = y.shape
    dx = torch.empty_like(y)
    check(_lib.lib().clipx_l2norm_bwd(rows, width, _p(_c(dy)), _p(y), _p(inv), _p(dx), _stream()))
    return dx


@family("loss")
def ce_rows(z, label_off, lse, weight, loss_acc):
    rows, cols = z.shape
    check(_lib.lib().clipx_ce_rows(rows, cols, _p(z), z.stride(0), label_off, _p(lse), float(weight), _p(loss_acc),
                                   _stream()))


@family("loss")
def ce_cols(z, lse, weight, loss_acc):
    rows, cols = z.shape
    check(_lib.lib().clipx_ce_cols(rows, cols, _p(z), z.stride(0), _p(lse), float(weight), _p(loss_acc), _stream()))


@family("loss")
def ce_grad(z, label_off, lse_row, w_row, lse_col, w_col, scale_dev, dscale_acc, col_label_off=0):
    rows, cols = z.shape
    check(_lib.lib().clipx_ce_grad(rows, cols, _p(z), z.stride(0), label_off, _p(lse_row), float(w_row), _p(lse_col),
                                   float(w_col), col_label_off, _p(scale_dev), _p(dscale_acc), _stream()))


FUSED_CE_DIMS = (16, 32, 64, 128, 256, 512, 640, 768, 1024)


@family("loss")
def ce_fused_fwd(P, Q, label_off, symmetric, w_own, w_oth, loss_acc):
    """Row (and, symmetric, column) log-sum-exps of z = P @ Q.T and the loss, without z in memory."""
    np_, E = P.shape
    nq = Q.shape[0]
    L = _lib.lib()
    nbytes = int(L.clipx_ce_fused_ws_bytes(np_, nq, int(symmetric)))
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=P.device)
    lse_own = torch.empty((np_,), dtype=torch.float32, device=P.device)
    lse_oth = torch.empty((nq,), dtype=torch.float32, device=P.device) if symmetric else None
    check(L.clipx_ce_fused_fwd(np_, nq, E, _p(_c(P)), _p(_c(Q)), int(label_off), int(symmetric), float(w_own), float(w_oth),
                               _p(lse_own), _p(lse_oth), _p(loss_acc), _p(ws), nbytes, _stream()))
    return lse_own, lse_oth


@family("loss")
def ce_fused_bwd(P, Q, lse_own, w_own, off_own, lse_oth, w_oth, off_oth, out_scale_dev, gout_dev, dscale_acc=None,
                 scale_dev=None):
    np_, E = P.shape
    dP = torch.empty((np_, E), dtype=torch.float32, device=P.device)
    nbytes = int(_lib.lib().clipx_ce_fused_bwd_ws_bytes(np_, Q.shape[0], E))
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=P.device)
    check(_lib.lib().clipx_ce_fused_bwd(np_, Q.shape[0], E, _p(_c(P)), _p(_c(Q)), _p(lse_own), float(w_own), int(off_own),
                                        _p(lse_oth), float(w_oth), int(off_oth), _p(out_scale_dev), 1.0, _p(gout_dev),
                                        _p(dP), _p(dscale_acc), _p(scale_dev), _p(ws), nbytes, _stream()))
    return dP


@family("loss")
def sigmoid_fused_fwd(A, B, scale_dev, bias_dev, pos_off, inv_r, want_grad, out3=None, dA=None):
    """SigLIP loss of z = scale * A @ B.T + bias without z in memory.  Returns (out3 = [loss, d(scale), d(bias)], dA or None);
    the gradients are at unit upstream gradient.  want_grad=False runs the loss-only walk.  Given out3 / dA are added to."""
    r, E = A.shape
    c = B.shape[0]
    L = _lib.lib()
    accumulate = out3 is not None
    assert not accumulate or (dA is not None) == bool(want_grad)
    nbytes = int(L.clipx_sigmoid_fused_ws_bytes(r, c, E, int(want_grad)))
    ws = torch.empty((max(nbytes, 16),), dtype=torch.uint8, device=A.device)
    if out3 is None:
        out3 = torch.empty((3,), dtype=torch.float32, device=A.device)
        dA = torch.empty((r, E), dtype=torch.float32, device=A.device) if want_grad else None
    check(L.clipx_sigmoid_fused_fwd(r, c, E, _p(_c(A)), _p(_c(B)), _p(scale_dev), _p(bias_dev), int(pos_off), float(inv_r),
                                    _p(out3), _p(dA), int(accumulate), _p(ws), nbytes, _stream()))
    return out3, dA


@family("loss")
def sigmoid_fused_bwd(A, B, scale_dev, bias_dev, pos_off, inv_r, gout_dev, dB=None, accumulate=False):
    """dB (+)= scale * upstream * dz.T @ A, the logits recomputed tile by tile."""
    r, E = A.shape
    c = B.shape[0]
    if dB is None:
        dB = torch.empty((c, E), dtype=torch.float32, device=A.device)
    L = _lib.lib()
    nbytes = int(L.clipx_sigmoid_fused_bwd_ws_bytes(r, c, E))
    ws = torch.empty((max(nbytes, 16),), dtype=torch.uint8, device=A.device)
    check(L.clipx_sigmoid_fused_bwd(r, c, E, _p(_c(A)), _p(_c(B)), _p(scale_dev), _p(bias_dev), int(pos_off), float(inv_r),
                                    _p(gout_dev), _p(_c(dB)), int(accumulate), _p(ws), nbytes, _stream()))
    return dB


@family("loss")
def sigmoid_dense(z, scale_dev, bias_dev, pos_off, inv_r):
    """In place: dot products z -> d(logits); returns [loss, d(scale), d(bias)] (unit upstream gradient)."""
    rows, cols = z.shape
    L = _lib.lib()
    nbytes = int(L.clipx_sigmoid_dense_ws_bytes(rows, cols))
    ws = torch.empty((max(nbytes, 16),), dtype=torch.uint8, device=z.device)
    out3 = torch.empty((3,), dtype=torch.float32, device=z.device)
    check(L.clipx_sigmoid_dense(rows, cols, _p(z), z.stride(0), _p(scale_dev), _p(bias_dev), int(pos_off), float(inv_r),
                                _p(out3), _p(ws), nbytes, _stream()))
    return out3


@family("loss")
def distill_fused_fwd(P, Q, TP, TQ, label_off, symmetric, w_own, w_oth, loss2):
    """Row (and, symmetric, column) statistics (lse_s, lse_t, X) of s = P @ Q.T and t = TP @ TQ.T without either in memory;
    loss2 += [contrastive, distill].  Returns (stats_own [3, np], stats_oth [3, nq] or None)."""
    np_, Es = P.shape
    nq, Et = Q.shape[0], TP.shape[1]
    assert Q.shape[1] == Es and TP.shape[0] == np_ and TQ.shape == (nq, Et)
    L = _lib.lib()
    nbytes = int(L.clipx_distill_fused_ws_bytes(np_, nq, int(symmetric)))
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=P.device)
    st_own = torch.empty((3, np_), dtype=torch.float32, device=P.device)
    st_oth = torch.empty((3, nq), dtype=torch.float32, device=P.device) if symmetric else None
    check(L.clipx_distill_fused_fwd(np_, nq, Es, Et, _p(_c(P)), _p(_c(Q)), _p(_c(TP)), _p(_c(TQ)), int(label_off),
                                    int(symmetric), float(w_own), float(w_oth), _p(st_own), _p(st_oth), _p(loss2), _p(ws),
                                    nbytes, _stream()))
    return st_own, st_oth


@family("loss")
def distill_fused_bwd(P, Q, TP, TQ, st_own, w_own, off_own, st_oth, w_oth, off_oth, gc_dev, gd_dev, out_scale_dev,
                      dscale_acc=None, scale_dev=None):
    """dP = osc * ds @ Q with ds recomputed tile by tile (both upstream gradients folded in)."""
    np_, Es = P.shape
    nq, Et = Q.shape[0], TP.shape[1]
    dP = torch.empty((np_, Es), dtype=torch.float32, device=P.device)
    L = _lib.lib()
    nbytes = int(L.clipx_distill_fused_bwd_ws_bytes(np_, nq, Es))
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=P.device)
    check(L.clipx_distill_fused_bwd(np_, nq, Es, Et, _p(_c(P)), _p(_c(Q)), _p(_c(TP)), _p(_c(TQ)), _p(st_own), float(w_own),
                                    int(off_own), _p(st_oth), float(w_oth), int(off_oth), _p(gc_dev), _p(gd_dev),
                                    _p(out_scale_dev), _p(dP), _p(dscale_acc), _p(scale_dev), _p(ws), nbytes, _stream()))
    return dP


@family("loss")
def distill_dense_fwd(s, t, label_off, symmetric, w_row, w_col, loss2):
    """Statistics and losses of materialised student / teacher logits [rows, cols]; returns (stats_row, stats_col or None)."""
    rows, cols = s.shape
    assert t.shape == s.shape
    L = _lib.lib()
    nbytes = int(L.clipx_distill_dense_ws_bytes(rows, cols))
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=s.device)
    st_row = torch.empty((3, rows), dtype=torch.float32, device=s.device)
    st_col = torch.empty((3, cols), dtype=torch.float32, device=s.device) if symmetric else None
    check(L.clipx_distill_dense_fwd(rows, cols, _p(s), s.stride(0), _p(t), t.stride(0), int(label_off), int(symmetric),
                                    float(w_row), float(w_col), _p(st_row), _p(st_col), _p(loss2), _p(ws), nbytes, _stream()))
    return st_row, st_col


@family("loss")
def distill_dense_grad(s, t, label_off, st_row, w_row, st_col, w_col, gc_dev, gd_dev, want_dt, scale_dev, tscale_dev,
                       dscales2):
    """In place s -> ds and (want_dt) t -> dt; dscales2 += [d(scale), d(teacher scale)]."""
    rows, cols = s.shape
    L = _lib.lib()
    nbytes = int(L.clipx_distill_dense_ws_bytes(rows, cols))
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=s.device)
    check(L.clipx_distill_dense_grad(rows, cols, _p(s), s.stride(0), _p(t), t.stride(0), int(label_off), _p(st_row),
                                     float(w_row), _p(st_col), float(w_col), _p(gc_dev), _p(gd_dev), int(want_dt),
                                     _p(scale_dev), _p(tscale_dev), _p(dscales2), _p(ws), nbytes, _stream()))


def scale_by_dev(x, s_dev, out=None):
    out = torch.empty_like(x) if out is None else out
    check(_lib.lib().clipx_scale_by_dev(x.numel(), _p(_c(x)), _p(s_dev), _p(out), _stream()))
    return out


# ------------------------------------------------------------------ parameters
@family("cast_weight")
def cast_weight(w, w16, wt16):
    N, K = w.shape
    check(_lib.lib().clipx_cast_weight(N, K, _p(_c(w)), _p(w16), _p(wt16), _stream()))


@family("cast_weight")
def quant_weight_e4m3(w, row_exp, w8, w16, wt16):
    """fp8 (e4m3, power-of-two scale per output channel) quantisation of a weight + its exact bf16 operand copies."""
    N, K = w.shape
    check(_lib.lib().clipx_quant_weight_e4m3(N, K, _p(_c(w)), _p(row_exp), _p(w8), _p(w16), _p(wt16), _stream()))


def quant_weight_multi(table, ntensors, blocks_rows, blocks_tiles, blocks_trows):
    check(_lib.lib().clipx_quant_weight_multi(_p(table), ntensors, blocks_rows, blocks_tiles, blocks_trows, _stream()))


def cast_weight_multi(table, ntensors, total_blocks):
    check(_lib.lib().clipx_cast_weight_multi(_p(table), ntensors, total_blocks, _stream()))


def adamw(p, g, m, v, lr, beta1, beta2, eps, wd, step, gscale=1.0):
    n = p.numel()
    bc1 = 1.0 - beta1 ** step
    bc2 = 1.0 - beta2 ** step
    check(_lib.lib().clipx_adamw(n, _p(p), _p(g), _p(m), _p(v), float(lr), float(beta1), float(beta2), float(eps),
                                 float(wd), float(bc1), float(bc2), float(gscale), _stream()))


@family("adamw")
def adamw_multi(table, ntensors, total_blocks, lr, beta1, beta2, eps, step, gscale=1.0):
    bc1 = 1.0 - beta1 ** step
    bc2 = 1.0 - beta2 ** step
    check(_lib.lib().clipx_adamw_multi(_p(table), int(ntensors), int(total_blocks), float(lr), float(beta1),
                                       float(beta2), float(eps), float(bc1), float(bc2), float(gscale), _stream()))


def sumsq(x, out):
    check(_lib.lib().clipx_sumsq(x.numel(), _p(x), _p(out), _stream()))


def clamp1(p, lo, hi):
    check(_lib.lib().clipx_clamp1(_p(p), float(lo), float(hi), _stream()))


def cast_f32_bf16(x, out, scale=1.0):
    assert x.dtype == torch.float32 and out.dtype == torch.bfloat16 and x.numel() == out.numel()
    assert out.is_contiguous(), "cast_f32_bf16 writes through out's pointer: out must be contiguous"
    check(_lib.lib().clipx_cast_f32_bf16(x.numel(), _p(_c(x)), _p(_c(out)), float(scale), _stream()))
    return out


def cast_bf16_f32(x, out, scale=1.0):
    assert x.dtype == torch.bfloat16 and out.dtype == torch.float32 and x.numel() == out.numel()
    assert out.is_contiguous(), "cast_bf16_f32 writes through out's pointer: out must be contiguous"
    check(_lib.lib().clipx_cast_bf16_f32(x.numel(), _p(_c(x)), _p(_c(out)), float(scale), _stream()))
    return out


def scale_(x, s):
    check(_lib.lib().clipx_scale(x.numel(), _p(x), float(s), _stream()))


# ------------------------------------------------------------------ token-level MaxSim (ColClipLoss)
def maxsim_reduce(S, q):
    """S [rows, groups*q] -> (maxv [rows, groups] fp32, arg [rows, groups] uint8)."""
    rows, cols = S.shape
    groups = cols // q
    maxv = torch.empty((rows, groups), dtype=torch.float32, device=S.device)
    arg = torch.empty((rows, groups), dtype=torch.uint8, device=S.device)
    check(_lib.lib().clipx_maxsim_reduce(dt_code(S.dtype), rows, groups, q, _p(_c(S)), _p(maxv), _p(arg), _stream()))
    return maxv, arg


def masked_mean(maxv, ct, n_tok):
    groups = maxv.shape[1]
    out = torch.empty((ct, groups), dtype=torch.float32, device=maxv.device)
    inv = torch.empty((ct, groups), dtype=torch.float32, device=maxv.device)
    check(_lib.lib().clipx_masked_mean(ct, n_tok, groups, _p(maxv), _p(out), _p(inv), _stream()))
    return out, inv


def maxsim_scatter(dlogits, inv_count, arg, n_tok, q, dtype, want_transpose):
    ct, groups = dlogits.shape
    P = torch.empty((ct * n_tok, groups * q), dtype=dtype, device=dlogits.device)
    PT = torch.empty((groups * q, ct * n_tok), dtype=dtype, device=dlogits.device) if want_transpose else None
    check(_lib.lib().clipx_maxsim_scatter(dt_code(dtype), ct, n_tok, groups, q, _p(_c(dlogits)), _p(inv_count), _p(arg),
                                          _p(P), _p(PT), _stream()))
    return P, PT


# fused form (bf16 tokens, >= 16 tokens per image): include/clipx.h "Fused MaxSim"
def _maxsim_count_text(txt):
    """txt [nt, n, e] bf16 -> (cnt int32 [nt], cu int32 [nt + 1]) on the device: the one launch of `clipx_maxsim_pack_text`"""
    nt, n, e = txt.shape
    cnt = torch.empty((nt,), dtype=torch.int32, device=txt.device)
    cu = torch.empty((nt + 1,), dtype=torch.int32, device=txt.device)
    check(_lib.lib().clipx_maxsim_pack_text(nt, n, e, _p(_c(txt)), _p(cnt), _p(cu), _stream()))
    return cnt, cu


def maxsim_pack_text(txt):
    """txt [nt, n, e] bf16 -> (cu int32 [nt+1] on the device, R = packed rows; one 4-byte read-back).  Trailing positions of a
    sample that are bitwise equal to its last position are folded into one representative row."""
    _, cu = _maxsim_count_text(txt)
    return cu, int(cu[txt.shape[0]].item())


def maxsim_text_counts(txt):
    """txt [nt, n, e] bf16 -> cnt int32 [nt]: the packed rows per sample as `maxsim_pack_text` counts them (leading rows + one
    representative of the bitwise-equal tail), without the read-back.  No samples: no launch."""
    if txt.shape[0] == 0:
        return torch.empty((0,), dtype=torch.int32, device=txt.device)
    return _maxsim_count_text(txt)[0]


def maxsim_pack_rows(txt, cu, R):
    nt, n, e = txt.shape
    packed = torch.empty((R, e), dtype=txt.dtype, device=txt.device)
    row_m = torch.empty((R,), dtype=torch.int32, device=txt.device)
    row_w = torch.empty((R,), dtype=torch.float32, device=txt.device)
    check(_lib.lib().clipx_maxsim_pack_rows(nt, n, e, _p(_c(txt)), _p(cu), _p(packed), _p(row_m), _p(row_w), _stream()))
    return packed, row_m, row_w


def maxsim_gemm(packed, img, ni, q, pmax, pidx, ldp):
    R, e = packed.shape
    check(_lib.lib().clipx_maxsim_gemm(R, ni, q, e, _p(_c(packed)), _p(_c(img)), _p(pmax), _p(pidx), ldp, _nt_stream()))


@family("gemm_nt.fwd_fp8")
def maxsim_gemm_fp8(packed8, packed_exp, img8, img_exp, ni, q, pmax, pidx, ldp):
    """the partials of `maxsim_gemm` from e4m3 rows with per-row exponents, on the fp8 MFMA"""
    R, e = packed8.shape
    assert packed8.dtype == torch.uint8 and img8.dtype == torch.uint8 and img8.shape == (ni * q, e)
    assert packed_exp.dtype == torch.int32 and packed_exp.numel() == R and img_exp.dtype == torch.int32 and img_exp.numel() == ni * q
    check(_lib.lib().clipx_maxsim_gemm_fp8(R, ni, q, e, _p(_c(packed8)), _p(_c(packed_exp)), _p(_c(img8)), _p(_c(img_exp)), _p(pmax),
                                           _p(pidx), ldp, _nt_stream()))


def maxsim_finish(R, ldp, r0, ld, ni, q, pmax, pidx, maxvT, argT):
    check(_lib.lib().clipx_maxsim_finish(R, ldp, r0, ld, ni, q, _p(pmax), _p(pidx), _p(maxvT), _p(argT), _stream()))


def maxsim_mean(nt, ni, ld, cu, row_w, maxvT):
    out = torch.empty((nt, ni), dtype=torch.float32, device=maxvT.device)
    inv = torch.empty((nt, ni), dtype=torch.float32, device=maxvT.device)
    check(_lib.lib().clipx_maxsim_mean(nt, ni, ld, _p(cu), _p(row_w), _p(maxvT), _p(out), _p(inv), _stream()))
    return out, inv


def maxsim_scatter_packed(R, r0, ld, ni, q, row_m, dlogits, inv_count, argT, P):
    check(_lib.lib().clipx_maxsim_scatter_packed(R, r0, ld, ni, q, _p(row_m), _p(_c(dlogits)), _p(inv_count), _p(argT), _p(P), _stream()))
    return P


def maxsim_scale_rows(x, row_w):
    y = torch.empty_like(x)
    check(_lib.lib().clipx_maxsim_scale_rows(x.shape[0], x.shape[1], _p(row_w), _p(_c(x)), _p(y), _stream()))
    return y


def maxsim_expand(dpacked, cu, nt, n_tok, dtype):
    e = dpacked.shape[1]
    out = torch.empty((nt, n_tok, e), dtype=dtype, device=dpacked.device)
    check(_lib.lib().clipx_maxsim_expand(dt_code(dtype), nt, n_tok, e, _p(cu), _p(_c(dpacked)), _p(out), _stream()))
    return out


# ------------------------------------------------------------------ retrieval evaluation
def retrieval_rank(scores, tgt_off, tgt_idx):
    """scores [R, C] fp32 (row stride allowed), CSR targets (int32) -> ranks [R] int32 (0 = first)."""
    rows, cols = scores.shape
    assert scores.dtype == torch.float32 and scores.stride(1) == 1
    ranks = torch.empty((rows,), dtype=torch.int32, device=scores.device)
    check(_lib.lib().clipx_retrieval_rank(rows, cols, _p(scores), scores.stride(0), _p(tgt_off), _p(tgt_idx), _p(ranks),
                                          _stream()))
    return ranks


# ------------------------------------------------------------------ late-interaction scoring (forward only)
MAXSIM_OPERAND_BYTES = (1 << 31) - 1     # one image chunk of the MaxSim GEMM stays addressable through a 2-GiB buffer descriptor
MAXSIM_MAX_IMAGES = 65535                # images per chunk
MAXSIM_TARGET_ROWS = 4096                # an image chunk is shrunk until a text chunk of this many packed rows fits the partials
MAXSIM_PARTIAL_BYTES = 2 << 30           # partial maxima (pmax + pidx) of one MaxSim GEMM: here and in the forward of loss._MaxSimFused
MAXSIM_GENERAL_BYTES = 2 << 30           # similarities of one chunk of the general route: here and in loss._MaxSimLogits


def maxsim_partial_ld(rows: int) -> int:
    """leading dimension of the partial arrays of a text chunk: its packed rows, rounded up to 64 bytes of fp32"""
    return (rows + 15) // 16 * 16


def maxsim_partial_rows(ci: int, q: int) -> int:
    """rows of the partial arrays of `ci` images (csrc/gemm_nt_maxsim.h): two segments per 64-column slot from 64 tokens per
    image up, two slot halves per image below that"""
    return 2 * ci if q < 64 else 2 * ((ci * q + 63) // 64)


def maxsim_partial_bytes(ci: int, q: int, rows: int) -> int:
    """pmax (fp32) + pidx (int16) of `ci` images against `rows` packed rows: 6 bytes per (row, 64-column slot, segment), per
    (row, image, slot half) below 64 tokens per image"""
    return 6 * maxsim_partial_rows(ci, q) * maxsim_partial_ld(rows)


def plan_maxsim_chunks(ni, q, e, cu_host, partial_bytes, operand_bytes=None, elem_bytes=2):
    """Chunk plan of `maxsim_scores` on the fused route; pure Python.  Returns (image_chunks, text_chunks):
      image_chunks [(k0, k1, ci)]: images k0 .. k1 go through the GEMM as `ci >= k1 - k0` images, the last ci - (k1 - k0) of
        them zero padding, with (ci * q) % 8 == 0 (GEMM alignment), ci <= 65535 and ci * q * e elements of `elem_bytes` bytes
        (2: bf16, 1: e4m3) below `operand_bytes`; only the last chunk can need padding;
      text_chunks [(m0, m1, r0, r1)]: runs of whole samples (packed rows cu[m0] = r0 .. cu[m1] = r1) whose partial arrays
        against the largest image chunk stay within `partial_bytes`; a single sample that does not fit is a chunk of its own.
    The image chunk is as large as the operand limit allows, but no larger than lets MAXSIM_TARGET_ROWS packed rows (or all of
    them) fit the partials: the GEMM wants a tall operand more than a wide one."""
    import math
    if operand_bytes is None:
        operand_bytes = MAXSIM_OPERAND_BYTES
    nt = len(cu_host) - 1
    unit = 8 // math.gcd(q, 8)                                   # image counts with (ci * q) % 8 == 0
    want_ld = maxsim_partial_ld(max(1, min(MAXSIM_TARGET_ROWS, cu_host[nt])))
    fit = partial_bytes // (12 * want_ld)                        # slots (q >= 64) or images whose partials fit
    cmax = min(MAXSIM_MAX_IMAGES, operand_bytes // (int(elem_bytes) * q * e), fit if q < 64 else fit * 64 // q)
    cmax = max(unit, cmax // unit * unit)
    cmax = min(cmax, (ni + unit - 1) // unit * unit)
    image_chunks = []
    for k0 in range(0, ni, cmax):
        k1 = min(ni, k0 + cmax)
        image_chunks.append((k0, k1, (k1 - k0 + unit - 1) // unit * unit))
    limit_rows = partial_bytes // (6 * maxsim_partial_rows(cmax, q)) // 16 * 16
    text_chunks, m0 = [], 0
    while m0 < nt:
        m1 = m0 + 1
        while m1 < nt and cu_host[m1 + 1] - cu_host[m0] <= limit_rows:
            m1 += 1
        text_chunks.append((m0, m1, cu_host[m0], cu_host[m1]))
        m0 = m1
    return image_chunks, text_chunks


def maxsim_score_fold(nm, ni, q, ldp, rbase, cu, m0, row_w, pmax, G, scores, alpha, scale):
    """Partials of one (image chunk, text chunk) -> scores[:ni, :nm] = scale * (alpha * G[:ni, :nm] + (1 - alpha) * tok^T);
    `G` and `scores` are views of the block (unit column stride).  pmax None: scale * G exactly."""
    assert scores.dtype == torch.float32 and scores.stride(1) == 1 and scores.shape[0] >= ni and scores.shape[1] >= nm
    if G is not None:
        assert G.dtype == torch.float32 and G.stride(1) == 1 and G.shape[0] >= ni and G.shape[1] >= nm
    cu_ptr = None if cu is None else cu.data_ptr() + 4 * m0
    check(_lib.lib().clipx_maxsim_score_fold(nm, ni, q, ldp, rbase, cu_ptr, _p(row_w), _p(pmax), _p(G),
                                             0 if G is None else G.stride(0), _p(scores), scores.stride(0), float(alpha),
                                             float(1.0 - alpha), float(scale), _stream()))
    return scores


def maxsim_gemm_takes(q: int, e: int, elem_bytes: int) -> bool:
    """whether the MaxSim GEMM takes `q` tokens per image of `e` elements of `elem_bytes` bytes (2: bf16, 1: e4m3)"""
    # the ping-pong engine (csrc/gemm_nt_pp.h) walks an operand row in k-steps of 128 bytes, 64 bf16 or 128 e4m3 elements, and its
    # pipeline needs at least two of them
    row_bytes = e * elem_bytes
    return 16 <= q <= 65535 and row_bytes % 128 == 0 and row_bytes >= 256


def maxsim_fused_applies(tok_img, tok_txt) -> bool:
    """the shapes `_MaxSimFused.applies` takes, without its image-count alignment (the chunk plan pads the last chunk)"""
    ni, q, e = tok_img.shape
    return (tok_txt.dtype == torch.bfloat16 and tok_img.dtype == torch.bfloat16 and tok_txt.is_cuda
            and maxsim_gemm_takes(q, e, 2) and os.environ.get("CLIPX_MAXSIM_FUSED", "1") != "0")


def _pack_text(txt):
    """bf16 text [nt, n, e] -> (packed [R, e], None, cu [nt + 1] int32, row_w [R]): the text operand of `_maxsim_scores_fused`"""
    txt = txt.contiguous()
    cu, R = maxsim_pack_text(txt)
    packed, _, row_w = maxsim_pack_rows(txt, cu, R)
    return packed, None, cu, row_w


def _rows_padded(x, r0, r1, rows):
    """x[r0:r1] as `rows` >= r1 - r0 rows: the view itself, or a copy with zero rows (byte 0, exponent 0) behind it"""
    if rows == r1 - r0:
        return x[r0:r1]
    op = torch.zeros((rows,) + tuple(x.shape[1:]), dtype=x.dtype, device=x.device)
    op[:r1 - r0] = x[r0:r1]
    return op


def _maxsim_scores_fused(img_rows, img_exp, packed, packed_exp, cu, row_w, ni, q, G, alpha, scale, out):
    """The fused route of `maxsim_scores` (exponents None: bf16 rows, `maxsim_gemm`) and of `maxsim_scores_fp8` (e4m3 bytes with
    one int32 exponent per row, `maxsim_gemm_fp8`).  img_rows [ni * q, e], packed [R, e]: the rows of `maxsim_pack_rows`."""
    e = img_rows.shape[1]
    dev = img_rows.device
    image_chunks, text_chunks = plan_maxsim_chunks(ni, q, e, cu.cpu().tolist(), MAXSIM_PARTIAL_BYTES,
                                                   elem_bytes=img_rows.element_size())
    cmax = max(c for _, _, c in image_chunks)
    ldmax = maxsim_partial_ld(max(r1 - r0 for _, _, r0, r1 in text_chunks))
    prow = maxsim_partial_rows(cmax, q)
    pmax = torch.empty((prow * ldmax,), dtype=torch.float32, device=dev)
    pidx = torch.empty((prow * ldmax,), dtype=torch.int16, device=dev)
    for k0, k1, ci in image_chunks:
        # zero images behind the last ones of a padded chunk: their columns are never folded
        op = _rows_padded(img_rows, k0 * q, k1 * q, ci * q)
        op_exp = None if img_exp is None else _rows_padded(img_exp, k0 * q, k1 * q, ci * q)
        for m0, m1, r0, r1 in text_chunks:
            ldp = maxsim_partial_ld(r1 - r0)
            if img_exp is None:
                maxsim_gemm(packed[r0:r1], op, ci, q, pmax, pidx, ldp)
            else:
                maxsim_gemm_fp8(packed[r0:r1], packed_exp[r0:r1], op, op_exp, ci, q, pmax, pidx, ldp)
            maxsim_score_fold(m1 - m0, k1 - k0, q, ldp, r0, cu, m0, row_w, pmax, None if G is None else G[k0:k1, m0:m1],
                              out[k0:k1, m0:m1], alpha, scale)
    return out


def _maxsim_scores_general(tok_img, tok_txt, G, alpha, scale, out):
    ni, q, e = tok_img.shape
    nt, n, _ = tok_txt.shape
    img = tok_img.contiguous().float().view(ni * q, e)
    txt = tok_txt.contiguous().float().view(nt * n, e)
    limit = MAXSIM_GENERAL_BYTES
    ci = max(1, min(ni, limit // max(1, 4 * n * q)))           # images per chunk: one sample's similarities fit
    ct = max(1, min(nt, limit // max(1, 4 * n * ci * q)))
    for k0 in range(0, ni, ci):
        k1 = min(ni, k0 + ci)
        cols = (k1 - k0) * q
        for m0 in range(0, nt, ct):
            m1 = min(nt, m0 + ct)
            rows = (m1 - m0) * n
            S = torch.empty((rows, cols), dtype=torch.float32, device=img.device)
            gemm_f32(rows, cols, e, txt[m0 * n:m1 * n], e, 1, img[k0 * q:k1 * q], 1, e, S, cols)
            maxv, _ = maxsim_reduce(S, q)
            del S
            tok, _ = masked_mean(maxv, m1 - m0, n)              # [m, k]
            blk = (1.0 - alpha) * tok.t()
            if G is not None:
                blk = alpha * G[k0:k1, m0:m1] + blk
            out[k0:k1, m0:m1] = scale * blk
    return out


def _maxsim_scores_frame(G, out, ni, nt, device):
    """the checks of `G` and `out` [ni, nt] fp32 that both scorers share -> (G with a unit column stride, out: allocated if None)"""
    if G is not None:
        assert G.shape == (ni, nt) and G.dtype == torch.float32
        if G.stride(1) != 1:
            G = G.contiguous()
    if out is None:
        out = torch.empty((ni, nt), dtype=torch.float32, device=device)
    assert out.shape == (ni, nt) and out.dtype == torch.float32 and out.stride(1) == 1
    return G, out


def maxsim_scores(tok_img, tok_txt, G, alpha, scale, out=None):
    """Late-interaction scores without autograd: scores [ni, nt] (fp32, image-major) =
        scale * (alpha * G + (1 - alpha) * MaxSim(tok_img [ni, q, e], tok_txt [nt, n, e])^T)
    with MaxSim the reference's compute_colbert_similarity (loss.py:20-46) and G [ni, nt] the fp32 global similarities (None:
    no global term).  bf16 tokens with q >= 16, e % 64 == 0 and e >= 128 go through the MaxSim GEMM and `clipx_maxsim_score_fold` per
    (image chunk x text chunk): nothing of size rows x images is kept.  Everything else (fp32 tokens, q < 16, other embed dims)
    runs in fp32 on gemm_f32 + maxsim_reduce + masked_mean.  alpha = 1 is scale * G bit for bit: no token kernel runs and the
    token features are not looked at (they may be None)."""
    alpha, scale = float(alpha), float(scale)
    if alpha == 1.0:
        assert G is not None, "maxsim_scores: alpha = 1 scores with the global similarities only and needs G"
        ni, nt = G.shape
    else:
        ni, q, e = tok_img.shape
        nt, n, e2 = tok_txt.shape
        assert e == e2 and tok_img.dtype == tok_txt.dtype and tok_img.is_cuda
    G, out = _maxsim_scores_frame(G, out, ni, nt, G.device if G is not None else tok_img.device)
    with torch.no_grad():
        if alpha == 1.0:
            for k0 in range(0, ni, 4 * MAXSIM_MAX_IMAGES):
                k1 = min(ni, k0 + 4 * MAXSIM_MAX_IMAGES)
                maxsim_score_fold(nt, k1 - k0, 0, 0, 0, None, 0, None, None, G[k0:k1], out[k0:k1], 1.0, scale)
            return out
        tok_img, tok_txt = tok_img.detach(), tok_txt.detach()
        if maxsim_fused_applies(tok_img, tok_txt):
            return _maxsim_scores_fused(tok_img.contiguous().view(ni * q, e), None, *_pack_text(tok_txt), ni, q, G, alpha, scale, out)
        return _maxsim_scores_general(tok_img, tok_txt, G, alpha, scale, out)


# ------------------------------------------------------------------ late-interaction scoring on e4m3 tokens
# Either side of `maxsim_scores_fp8` is a bf16 tensor (quantised on the fly) or its stored form: an image side (bytes [ni, q, e]
# uint8, exp [ni, q] int32), a text side (bytes [nt, n, e], exp [nt, n], cnt [nt] int32) with cnt = `maxsim_text_counts` of the
# bf16 rows, as a tuple or a list.  The quantiser works row by row, so the packed rows of a stored text side are the rows the
# on-the-fly route quantises after packing, byte for byte.
def _image_side(x):
    """image side -> (tokens [ni, q, e] bf16 or bytes uint8, exp [ni, q] int32 of the stored form or None)"""
    if isinstance(x, (tuple, list)):
        return x[0], x[1]
    return x, None


def _text_side(x):
    """text side -> (tokens [nt, n, e] bf16 or bytes uint8, exp [nt, n] of the stored form or None, cnt [nt] or None)"""
    if isinstance(x, (tuple, list)):
        return x[0], x[1], x[2] if len(x) > 2 else None
    return x, None, None


def maxsim_fp8_applies(img, txt) -> bool:
    """whether `maxsim_scores_fp8` runs the fp8 MaxSim GEMM on these sides (else: the general fp32 route on dequantised values)"""
    ti, ie = _image_side(img)
    tt, te, _ = _text_side(txt)
    ni, q, e = ti.shape
    ok_i = ti.dtype == (torch.bfloat16 if ie is None else torch.uint8)
    ok_t = tt.dtype == (torch.bfloat16 if te is None else torch.uint8)
    return (ok_i and ok_t and ti.is_cuda and tt.is_cuda and maxsim_gemm_takes(q, e, 1)
            and os.environ.get("CLIPX_MAXSIM_FUSED", "1") != "0")


def _pack_text_quantised(txt):
    """bf16 text -> (packed8 [R, e], packed_exp [R], cu, row_w): the packed rows, quantised row by row"""
    packed, _, cu, row_w = _pack_text(txt)
    return quant_rows_e4m3(packed) + (cu, row_w)


def _fp8_pack_stored_text(t8, te, cnt):
    """stored text side -> (packed8 [R, e], packed_exp [R], cu [nt + 1] int32, row_w [R]): the rows `maxsim_pack_rows` picks"""
    nt, n, e = t8.shape
    cu = torch.zeros((nt + 1,), dtype=torch.int32, device=t8.device)
    cu[1:] = torch.cumsum(cnt, 0)
    R = int(cu[nt].item())
    packed, row_m, row_w = maxsim_pack_rows(t8.contiguous().view(torch.bfloat16), cu, R)        # a byte row as e / 2 bf16: a copy
    pos = torch.arange(R, dtype=torch.int64, device=t8.device) - cu[:-1].long()[row_m.long()]
    return packed.view(torch.uint8), te.contiguous().view(-1)[row_m.long() * n + pos].contiguous(), cu, row_w


def maxsim_scores_fp8(img, txt, G, alpha, scale, out=None):
    """`maxsim_scores` on e4m3 token features: the same contract and output, scores [ni, nt] fp32 image-major =
        scale * (alpha * G + (1 - alpha) * MaxSim(dequantised img, dequantised txt)^T).
    Each side is a bf16 tensor (quantised here, per token row) or its stored form, (bytes, exp) for images and (bytes, exp, cnt)
    for texts (see above).  With 16 <= q, e % 128 == 0 and e >= 256 on the device the MaxSim GEMM runs on the fp8 MFMA
    (`clipx_maxsim_gemm_fp8`; products exact, sums fp32, both exponents applied before the maximum) and
    `clipx_maxsim_score_fold` finishes as on the bf16 route.  Otherwise (`maxsim_fp8_applies` is False) the quantised
    operands are dequantised to fp32 and scored by the general route: the same numbers up to summation order.  alpha = 1 is
    scale * G bit for bit; no token kernel runs and the token sides are not looked at."""
    alpha, scale = float(alpha), float(scale)
    if alpha == 1.0:
        return maxsim_scores(None, None, G, 1.0, scale, out=out)
    ti, ie = _image_side(img)
    tt, te, cnt = _text_side(txt)
    ni, q, e = ti.shape
    nt, n, e2 = tt.shape
    assert e == e2 and ti.device == tt.device
    G, out = _maxsim_scores_frame(G, out, ni, nt, ti.device)
    with torch.no_grad():
        fused = maxsim_fp8_applies(img, txt)
        if ie is None:
            ti, ie = quant_tokens_e4m3(ti.detach())
        if fused:
            text = _pack_text_quantised(tt.detach()) if te is None else _fp8_pack_stored_text(tt, te, cnt)
            return _maxsim_scores_fused(ti.contiguous().view(ni * q, e), ie.contiguous().view(ni * q), *text, ni, q, G, alpha, scale, out)
        if te is None:
            tt, te = quant_tokens_e4m3(tt.detach())
        return _maxsim_scores_general(dequant_tokens_e4m3(ti, ie), dequant_tokens_e4m3(tt, te), G, alpha, scale, out)


# ------------------------------------------------------------------ gathered MaxSim (late-interaction reranking)
MAXSIM_PAIRS_ROWS = 80                   # query rows `clipx_maxsim_pairs` stages: five 16-row tiles of accumulators (MSP_QT)
MAXSIM_PAIRS_STAGE_BYTES = 128 << 10     # ... and their bytes in LDS, rows padded to 16 and to e + 8 elements (MSP_LDS_BYTES)


def maxsim_pairs_takes(q: int, n: int, e: int, gallery_is_image=None) -> bool:
    """Whether `clipx_maxsim_pairs` (csrc/maxsim_pairs.hip) scores pairs of images of `q` and texts of `n` tokens of `e` bf16
    elements.  The rule of the bf16 fused route, e % 64 == 0, e >= 128 and q >= 16 (the kernel walks a row in 32-element MFMA steps
    and masks, not skips, a partial 16-row tile), and the kernel's own limit: the QUERY side is staged whole in LDS and held in five
    16-row accumulator tiles, so it has at most 80 rows and 16-padded rows x (e + 8) x 2 bytes <= 128 KiB.  The query side is the
    text (n rows) over an image gallery and the image (q rows) over a text gallery; `gallery_is_image=None` asks for both
    directions.  The gallery side streams and has no limit."""
    if not (e % 64 == 0 and e >= 128 and q >= 16 and n >= 1):
        return False
    sides = {True: (n,), False: (q,), None: (q, n)}[gallery_is_image]
    return all(r <= MAXSIM_PAIRS_ROWS and (r + 15) // 16 * 16 * (e + 8) * 2 <= MAXSIM_PAIRS_STAGE_BYTES for r in sides)


def _pair_chunks(gallery_chunks):
    """[tokens or (tokens, cnt or None)] -> ([tokens], [cnt or None])"""
    toks, cnts = [], []
    for c in gallery_chunks:
        t, cnt = (c[0], c[1] if len(c) > 1 else None) if isinstance(c, (tuple, list)) else (c, None)
        toks.append(t)
        cnts.append(cnt)
    return toks, cnts


def _maxsim_pairs_general(query_tokens, toks, chunk_items, cand, Gp, alpha, scale, gallery_is_image, out):
    """The plain route of `maxsim_pair_scores`: torch on the device in fp32, over query chunks whose gathered tokens and
    similarities stay within MAXSIM_GENERAL_BYTES: gather, einsum, max, masked mean over all n text rows (the rows of a
    bitwise-equal tail have equal maxima, so this is the weighted mean of the packed rows up to summation order)."""
    nq, C = cand.shape
    rows_g, e = toks[0].shape[1], toks[0].shape[2]
    rows_q = query_tokens.shape[1]
    per_query = 4 * C * (rows_g * e + 2 * rows_g * rows_q)
    step = max(1, min(nq, MAXSIM_GENERAL_BYTES // max(1, per_query)))
    for a in range(0, nq, step):
        b = min(nq, a + step)
        pos = cand[a:b].long()
        live = pos >= 0
        p = pos.clamp(min=0)
        g = torch.zeros((b - a, C, rows_g, e), dtype=torch.float32, device=cand.device)
        for ci, t in enumerate(toks):
            m = live & (p // chunk_items == ci)
            g[m] = t[(p[m] - ci * chunk_items)].float()
        qt = query_tokens[a:b].float()
        if gallery_is_image:
            sim = torch.einsum("mnd,mcqd->mcnq", qt, g)
        else:
            sim = torch.einsum("mcnd,mqd->mcnq", g, qt)
        mx = sim.max(dim=3)[0]
        del sim, g
        tok = mx.sum(-1) / ((mx != 0).to(torch.float32).sum(-1) + 1e-8)
        blk = (1.0 - alpha) * tok
        if Gp is not None:
            blk = alpha * Gp[a:b] + blk
        out[a:b] = torch.where(live, scale * blk, torch.full_like(blk, float("-inf")))
    return out


def maxsim_pair_scores(query_tokens, gallery_chunks, chunk_items, cand, Gp, alpha, scale, gallery_is_image, out=None):
    """Late-interaction scores of chosen (query, gallery item) pairs: out [nq, C] fp32,
        out[i, c] = scale * (alpha * Gp[i, c] + (1 - alpha) * MaxSim(pair i, cand[i, c])),     -inf where cand[i, c] == -1
    with MaxSim as in `maxsim_scores`.  query_tokens [nq, rows, e] is one tensor; the gallery is its chunked storage as it is:
    `gallery_chunks` lists the token tensors [items, rows, e] (the last one may hold fewer than `chunk_items` items), for a bf16
    text gallery (tokens, cnt) with cnt = `maxsim_text_counts` of the chunk (computed here when missing); position p is item
    p % chunk_items of chunk p // chunk_items.  gallery_is_image: the queries are texts and the gallery holds images, else the
    other way round.  cand [nq, C] int, contiguous; Gp [nq, C] fp32 global similarities of the pairs or None (no global term).
    bf16 tokens of a shape `maxsim_pairs_takes` go through `clipx_maxsim_pairs`: nothing is gathered or packed.  Everything
    else -- fp32 tokens, other shapes, CLIPX_MAXSIM_FUSED=0 -- takes the plain torch route in fp32: the same numbers up to
    summation order.  alpha = 1 is scale * Gp (bit for bit) and reads no tokens."""
    alpha, scale = float(alpha), float(scale)
    if cand.dim() != 2 or cand.dtype not in (torch.int32, torch.int64):
        raise ValueError("maxsim_pair_scores: cand must be [nq, C] int32 or int64")
    nq, C = cand.shape
    if (C > 1 and cand.stride(1) != 1) or (nq > 1 and cand.stride(0) != C):
        raise ValueError(f"maxsim_pair_scores: cand must be contiguous (strides {tuple(cand.stride())} for shape {(nq, C)})")
    dev = cand.device
    if Gp is not None:
        if Gp.shape != (nq, C) or Gp.dtype != torch.float32 or (C > 1 and Gp.stride(1) != 1):
            raise ValueError("maxsim_pair_scores: Gp must be [nq, C] fp32 with a unit column stride")
    if out is None:
        out = torch.empty((nq, C), dtype=torch.float32, device=dev)
    if out.shape != (nq, C) or out.dtype != torch.float32 or (C > 1 and out.stride(1) != 1):
        raise ValueError("maxsim_pair_scores: out must be [nq, C] fp32 with a unit column stride")
    if nq == 0 or C == 0:
        return out
    with torch.no_grad():
        if alpha == 1.0:
            if Gp is None:
                raise ValueError("maxsim_pair_scores: alpha = 1 scores with the global similarities only and needs Gp")
            torch.mul(Gp, scale, out=out)
            out.masked_fill_(cand < 0, float("-inf"))
            return out
        toks, cnts = _pair_chunks(gallery_chunks)
        n_items = (len(toks) - 1) * int(chunk_items) + toks[-1].shape[0] if toks else 0
        if any(t.shape[0] != chunk_items for t in toks[:-1]) or (toks and not 1 <= toks[-1].shape[0] <= chunk_items):
            raise ValueError("maxsim_pair_scores: every chunk but the last holds chunk_items items")
        if not toks:
            if bool((cand != -1).any()):
                raise ValueError("maxsim_pair_scores: a candidate position in an empty gallery")
            return out.fill_(float("-inf"))
        query_tokens = query_tokens.detach()
        q, n = (toks[0].shape[1], query_tokens.shape[1]) if gallery_is_image else (query_tokens.shape[1], toks[0].shape[1])
        e = query_tokens.shape[2]
        if query_tokens.shape[0] != nq or any(t.shape[1:] != toks[0].shape[1:] or t.dtype != query_tokens.dtype for t in toks) \
                or toks[0].shape[2] != e:
            raise ValueError("maxsim_pair_scores: token shapes or dtypes of the query and the gallery chunks disagree")
        fused = (query_tokens.dtype == torch.bfloat16 and query_tokens.is_cuda and maxsim_pairs_takes(q, n, e, bool(gallery_is_image))
                 and os.environ.get("CLIPX_MAXSIM_FUSED", "1") != "0")
        if not fused:
            if bool(((cand < -1) | (cand >= n_items)).any()):
                raise ValueError(f"maxsim_pair_scores: a candidate position lies outside [0, {n_items}) and is not -1")
            return _maxsim_pairs_general(query_tokens, toks, int(chunk_items), cand, Gp, alpha, scale, bool(gallery_is_image), out)
        query_tokens = query_tokens.contiguous()
        cand32 = cand if cand.dtype == torch.int32 else cand.to(torch.int32)
        query_cnt = gal_cnt = None
        if gallery_is_image:
            query_cnt = maxsim_text_counts(query_tokens)
        else:
            cnts = [c if c is not None else maxsim_text_counts(t.contiguous()) for t, c in zip(toks, cnts)]
            assert all(c.dtype == torch.int32 and c.is_contiguous() and c.shape[0] >= t.shape[0] for t, c in zip(toks, cnts))
            gal_cnt = torch.tensor([c.data_ptr() for c in cnts], dtype=torch.int64, device=dev)
        gal_tok = torch.tensor([_p(_c(t)) for t in toks], dtype=torch.int64, device=dev)
        status = torch.empty((1,), dtype=torch.int32, device=dev)
        ld = (lambda t: t.stride(0)) if nq > 1 else (lambda t: C)        # the stride of a dimension of one element says nothing
        check(_lib.lib().clipx_maxsim_pairs(1 if gallery_is_image else 0, nq, C, q, n, e, _p(query_tokens), _p(query_cnt), _p(gal_tok),
                                            _p(gal_cnt), len(toks), int(chunk_items), n_items, _p(cand32), C, _p(Gp),
                                            0 if Gp is None else ld(Gp), _p(out), ld(out), alpha, float(1.0 - alpha),
                                            scale, _p(status), _stream()))
        return out


# ------------------------------------------------------------------ streaming top-k (late-interaction search)
TOPK_MAX_K = 256


def topk_init(nq, k, device):
    """Empty running lists of `topk_merge`: (best_val [nq, k] fp32 of -inf, best_idx [nq, k] int32 of -1)."""
    if not 1 <= k <= TOPK_MAX_K:
        raise ValueError(f"topk_init: k must be in 1 .. {TOPK_MAX_K} (got {k})")
    return (torch.full((nq, k), float("-inf"), dtype=torch.float32, device=device),
            torch.full((nq, k), -1, dtype=torch.int32, device=device))


def topk_merge(scores, query_dim, c_base, best_val, best_idx):
    """One step of the running selection (`clipx_topk_merge`): `scores` is a 2-D fp32 view whose dimension `query_dim` (0 or 1)
    indexes the queries and whose other dimension indexes gallery positions c_base, c_base + 1, ...; one of its strides must
    be 1.  best_val / best_idx [nq, k] are updated in place: the k best under (larger value, then smaller position)."""
    assert query_dim in (0, 1) and scores.dim() == 2 and scores.dtype == torch.float32
    nq, nc = scores.shape[query_dim], scores.shape[1 - query_dim]
    qs, cs = scores.stride(query_dim), scores.stride(1 - query_dim)
    if nq == 1 and nc > 1:                                       # the stride of a dimension of one element says nothing
        qs = 1 if cs != 1 else max(2, nc)
    elif nc == 1 and nq > 1:
        cs = 1 if qs != 1 else max(2, nq)
    k = best_val.shape[1] if best_val.dim() == 2 else 0
    assert best_val.shape == (nq, k) and best_idx.shape == (nq, k)
    assert best_val.dtype == torch.float32 and best_idx.dtype == torch.int32
    check(_lib.lib().clipx_topk_merge(nq, nc, k, _p(scores), qs, cs, int(c_base), _p(_c(best_val)), _p(_c(best_idx)), _stream()))
    return best_val, best_idx
