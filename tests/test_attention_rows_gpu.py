"""Every attention entry point of the C ABI against the fp64 reference of tests/attention_ref.py, element by element:
|got - ref| <= C u A with each element's own amplification A (see that module), instead of one scalar scaled to the
tensor's largest entry.  The entry points are called through _lib.lib() directly, as ops.py calls them, but every output is
the interior of a buffer with GUARD rows in front and behind and NaN everywhere: afterwards the guards hold their prefill
bit for bit (nothing written outside), the interior is finite (no row skipped: ops.py hands the kernels torch.empty, where a
skipped row reads as whatever the allocator left there), every part is inside the bound and the elements that no gradient
reaches are exactly zero.  The reference is never another kernel.

Which kernel a shape runs on is asserted where the ABI exposes the choice (clipx_attention_lse_supported,
clipx_attention_pooled_supported, TextLayout.buckets); the other dispatch lines are named beside the cases."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from colxlip_amd import _lib, ops  # noqa: E402
from colxlip_amd.ops import _stream, check, dt_code  # noqa: E402
from tests import attention_ref as R  # noqa: E402

DEV = "cuda"
GUARD = 64
B, H = R.BATCH, R.HEADS


# ---------------------------------------------------------------------------------------------------------- plumbing
class Guarded:
    """[rows, cols] of dtype inside a NaN-filled buffer with GUARD rows on either side"""

    def __init__(self, rows, cols, dtype):
        self.buf = torch.full((rows + 2 * GUARD, cols), float("nan"), dtype=dtype, device=DEV)
        self.t = self.buf[GUARD:GUARD + rows]
        self.rows = rows

    def ptr(self):
        return self.t.data_ptr()

    def guards_intact(self) -> bool:
        as_int = torch.int16 if self.buf.dtype == torch.bfloat16 else torch.int32
        bits = self.buf.view(as_int)
        fill = torch.full((1,), float("nan"), dtype=self.buf.dtype, device=DEV).view(as_int)
        return bool((bits[:GUARD] == fill).all()) and bool((bits[GUARD + self.rows:] == fill).all())


def _dev(x, dtype=None):
    x = x.to(DEV)
    return x.to(dtype).contiguous() if dtype is not None else x.contiguous()


class Report:
    """collects what went wrong over the families of one case, and the largest ratio per part for the printed record"""

    def __init__(self, case):
        self.case, self.bad, self.peak = case, [], {}

    def parts(self, where, got, ref_parts, amp, u, c):
        for p, v in R.ratios(got, ref_parts, amp, u).items():
            self.peak[p] = max(self.peak.get(p, 0.0), v)
            if not bool(torch.isfinite(got[p].float()).all()):
                self.bad.append(f"{where}: {p} is not finite (a row the kernel did not write?)")
            elif not v <= c:
                self.bad.append(f"{where}: {p} ratio {v:.3g} > {c:g}")

    def lse(self, where, got, ref, amp, sums_rounded_p):
        unit, c = R.lse_unit(amp, sums_rounded_p)
        v = R.ratio(got, ref, unit, 1.0)
        self.peak["lse"] = max(self.peak.get("lse", 0.0), v)
        if not v <= c:
            self.bad.append(f"{where}: lse ratio {v:.3g} > {c:g}")

    def guards(self, where, *bufs):
        for i, b in enumerate(bufs):
            if not b.guards_intact():
                self.bad.append(f"{where}: guard rows of output {i} were written")

    def expect(self, where, ok, what):
        if not ok:
            self.bad.append(f"{where}: {what}")

    def finish(self):
        print(f"ratios {self.case}: " + "  ".join(f"{p} {v:.3g}" for p, v in self.peak.items()))
        assert not self.bad, "\n".join(self.bad)


# ---------------------------------------------------------------------------------------------------------- dense
def _dense_two_sweep(dtype, qkv, dout, batch, L, heads, hd, causal):
    lib, d = _lib.lib(), heads * hd
    out, dqkv = Guarded(batch * L, d, dtype), Guarded(batch * L, 3 * d, dtype)
    check(lib.clipx_attention_fwd(dt_code(dtype), batch, L, heads, hd, int(causal), qkv.data_ptr(), out.ptr(), _stream()))
    check(lib.clipx_attention_bwd(dt_code(dtype), batch, L, heads, hd, int(causal), qkv.data_ptr(), dout.data_ptr(), dqkv.ptr(),
                                  _stream()))
    return out, dqkv


def _dense_handover(dtype, qkv, dout, batch, L, heads, hd, causal):
    lib, d = _lib.lib(), heads * hd
    out, dqkv = Guarded(batch * L, d, dtype), Guarded(batch * L, 3 * d, dtype)
    lse = Guarded(batch * heads, L, torch.float32)
    check(lib.clipx_attention_fwd_lse(dt_code(dtype), batch, L, heads, hd, int(causal), qkv.data_ptr(), out.ptr(), lse.ptr(),
                                      _stream()))
    check(lib.clipx_attention_bwd_lse(dt_code(dtype), batch, L, heads, hd, int(causal), qkv.data_ptr(), dout.data_ptr(), out.ptr(),
                                      lse.ptr(), dqkv.ptr(), _stream()))
    return out, dqkv, lse


# Which kernel each group runs on (csrc/attention.hip):
#   f32_whole      dispatch(): 2 L hd floats fit LDS and hd in {32, 64, 80}      -> launch_f32<hd>
#   f32_generic    dispatch(): hd = 128, or L = 700 at hd 64 (358 KiB > 160 KiB) -> dispatch_gen<float>
#   bf16_whole     dispatch_bf16(): hd = 64, L <= 128 -> launch_bf16<2 | 4 | 6 | 8> by L <= 32 | 64 | 96 | 128; a length that
#                  leaves whole tiles of the instantiation empty (16, 33, 65, 97) takes its guarded (PACKED) form
#   bf16_online64  bf16_long_applies(): hd = 64, 128 < L <= 608 -> launch_bf16_long<64>; 8-wave blocks up to L = 320, one
#                  block of nt waves from 321
#   bf16_online80  bf16_long_applies(): hd = 80, L <= 288      -> launch_bf16_long<80>
#   bf16_generic   dispatch_bf16(): everything else (hd 64 L = 609, hd 80 L = 289, hd 128, hd 32) -> dispatch_gen<bf16_t>
# bf16_long_applies() is what clipx_attention_lse_supported returns, so the online-softmax groups are asserted below.
@pytest.mark.parametrize("group,dtype,hd,L,causal", list(R.dense_cases()),
                         ids=[f"{g}-hd{hd}-L{L}-{'causal' if c else 'full'}" for g, _, hd, L, c in R.dense_cases()])
def test_dense_entry_points(group, dtype, hd, L, causal):
    rep = Report(f"{group} hd{hd} L{L} causal={int(causal)}")
    u, c = R.unit(dtype), (R.C_BF16 if dtype == torch.bfloat16 else R.C_F32)
    handover = bool(_lib.lib().clipx_attention_lse_supported(dt_code(dtype), L, hd))
    assert handover == (group in R.ONLINE_GROUPS)
    for make in R.FAMILIES:
        qkv, dout = (_dev(t, dtype) for t in make(B, L, H, hd))
        ref = R.reference(qkv, dout, B, L, H, causal)
        out, dqkv = _dense_two_sweep(dtype, qkv, dout, B, L, H, hd, causal)
        rep.guards(f"{make.__name__} fwd/bwd", out, dqkv)
        rep.parts(f"{make.__name__} fwd/bwd", R.parts_of(out.t, dqkv.t), ref.parts, ref.amp, u, c)
        if handover:
            out2, dqkv2, lse = _dense_handover(dtype, qkv, dout, B, L, H, hd, causal)
            rep.guards(f"{make.__name__} fwd_lse/bwd_lse", out2, dqkv2, lse)
            rep.parts(f"{make.__name__} fwd_lse/bwd_lse", R.parts_of(out2.t, dqkv2.t), ref.parts, ref.amp, u, c)
            rep.lse(f"{make.__name__} fwd_lse", lse.t, ref.lse, ref.lse_amp, True)
    rep.finish()


# ---------------------------------------------------------------------------------------------------------- packed rows
def _captions(batch, L, vocab, seed, min_len):
    """token ids with one EOT (= vocab - 1) per row at a seeded position >= min_len - 1, zeros behind it; the first caption
    has L tokens, the last min_len"""
    g = torch.Generator().manual_seed(seed)
    text = torch.randint(1, vocab - 2, (batch, L), generator=g)
    eot = torch.randint(min_len - 1, L, (batch,), generator=g)
    eot[0], eot[batch - 1] = L - 1, min_len - 1
    pos = torch.arange(L).unsqueeze(0)
    text = torch.where(pos < eot.unsqueeze(1), text, torch.zeros_like(text))
    text[torch.arange(batch), eot] = vocab - 1
    return text, eot + 1


# dispatch_packed() (csrc/attention.hip): bf16 -> launch_bf16<2 | 4 | 6 | 8> with cu_rows by the bucket's max_len, fp32 ->
# launch_f32<hd> with cu_rows.  Context 128 with captions of 97 .. 128 tokens puts every caption into a bucket of
# max_len > 96, which is launch_bf16<8>.
@pytest.mark.parametrize("batch", [5, 300])
@pytest.mark.parametrize("dtype,hd,context,min_len", [(torch.bfloat16, 64, 77, 2), (torch.bfloat16, 64, 128, 97),
                                                      (torch.float32, 32, 77, 2), (torch.float32, 64, 77, 2),
                                                      (torch.float32, 80, 77, 2)],
                         ids=["bf16-hd64-ctx77", "bf16-hd64-ctx128", "f32-hd32", "f32-hd64", "f32-hd80"])
def test_packed_entry_points(dtype, hd, context, min_len, batch):
    """every caption of a TextLayout against the reference of that caption alone; the filler sequences behind the live rows
    (zero dO) get exactly zero gradients"""
    lib, d, vocab = _lib.lib(), H * hd, 500
    text, lens = _captions(batch, context, vocab, seed=7 + batch, min_len=min_len)
    lay = ops.TextLayout(text.to(DEV), vocab)
    cu = lay.cu[:lay.nseq + 1].cpu().tolist()
    assert cu[-1] == lay.rows and [cu[s + 1] - cu[s] for s in range(batch)] == lens.tolist()
    if min_len == 97:
        first, count, cap = lay.buckets[-1]                # the 8-tile bucket holds every caption (ids below batch: not a filler)
        assert cap == 128 and int((lay.order[first:first + count] < batch).sum()) == batch
    elif batch == 300:
        assert [cap for _, _, cap in lay.buckets] == [32, 64, 77]
    u, c = R.unit(dtype), (R.C_BF16 if dtype == torch.bfloat16 else R.C_F32)
    rep = Report(f"packed {str(dtype)[6:]} hd{hd} ctx{context} b{batch}")
    for causal in (False, True):
        for make in R.FAMILIES:
            qkv, dout = (_dev(t, dtype) for t in make(1, lay.rows, H, hd))
            dout[lay.rows_live:] = 0
            ref_parts, amp = R.packed_reference(qkv, dout, cu, H, causal)
            out, dqkv = Guarded(lay.rows, d, dtype), Guarded(lay.rows, 3 * d, dtype)
            for first, count, max_len in lay.buckets:
                check(lib.clipx_attention_packed_fwd(dt_code(dtype), count, max_len, H, hd, int(causal),
                                                     lay.order.data_ptr() + 4 * first, lay.cu.data_ptr(), qkv.data_ptr(), out.ptr(),
                                                     _stream()))
                check(lib.clipx_attention_packed_bwd(dt_code(dtype), count, max_len, H, hd, int(causal),
                                                     lay.order.data_ptr() + 4 * first, lay.cu.data_ptr(), qkv.data_ptr(),
                                                     dout.data_ptr(), dqkv.ptr(), _stream()))
            where = f"{make.__name__} causal={int(causal)}"
            rep.guards(where, out, dqkv)
            rep.parts(where, R.parts_of(out.t, dqkv.t), ref_parts, amp, u, c)
            rep.expect(where, not bool((dqkv.t[lay.rows_live:] != 0).any()), "filler rows have a gradient")
    rep.finish()


# ---------------------------------------------------------------------------------------------------------- pooled row
def _pooled(split, qkv, dout, idx, cu, nseq, L, max_len, heads, hd, causal):
    """(out, lse, dq or None, dkv or dqkv) of the fused or the split entry points, all guarded"""
    lib, d, rows, dt = _lib.lib(), heads * hd, qkv.shape[0], dt_code(qkv.dtype)
    cu_p = cu.data_ptr() if cu is not None else None
    Lk = 0 if cu is not None else L
    out, lse = Guarded(nseq, d, qkv.dtype), Guarded(nseq * heads, 1, torch.float32)
    if not split:
        dqkv = Guarded(rows, 3 * d, qkv.dtype)
        check(lib.clipx_attention_pooled_fwd(dt, nseq, Lk, max_len, heads, hd, int(causal), qkv.data_ptr(), idx.data_ptr(), cu_p,
                                             out.ptr(), lse.ptr(), _stream()))
        check(lib.clipx_attention_pooled_bwd(dt, nseq, Lk, max_len, heads, hd, int(causal), qkv.data_ptr(), dout.data_ptr(),
                                             lse.ptr(), idx.data_ptr(), cu_p, dqkv.ptr(), _stream()))
        return out, lse, None, dqkv
    q, kv = qkv[idx.long(), :d].contiguous(), qkv[:, d:].contiguous()
    dq, dkv = Guarded(nseq, d, qkv.dtype), Guarded(rows, 2 * d, qkv.dtype)
    check(lib.clipx_attention_pooled_fwd_split(dt, nseq, Lk, max_len, heads, hd, int(causal), q.data_ptr(), kv.data_ptr(),
                                               idx.data_ptr(), cu_p, out.ptr(), lse.ptr(), _stream()))
    check(lib.clipx_attention_pooled_bwd_split(dt, nseq, Lk, max_len, heads, hd, int(causal), q.data_ptr(), kv.data_ptr(),
                                               dout.data_ptr(), lse.ptr(), idx.data_ptr(), cu_p, dq.ptr(), dkv.ptr(), _stream()))
    return out, lse, dq, dkv


def _pooled_case(rep, where, qkv, dout, idx, cu, nseq, L, max_len, hd, causal, ref_parts, amp, ref_lse, lse_amp):
    """fused and split entry points against the reference, and against each other bit for bit: launch_pooled() runs the
    same kernel on both, ApAddr only moves the addresses, so the arithmetic is the same operation for operation."""
    d = H * hd
    at = idx.long()
    out, lse, _, dqkv = _pooled(False, qkv, dout, idx, cu, nseq, L, max_len, H, hd, causal)
    rep.guards(f"{where} fused", out, lse, dqkv)
    got = {"o": out.t, "dq": dqkv.t[:, :d], "dk": dqkv.t[:, d:2 * d], "dv": dqkv.t[:, 2 * d:]}
    want = dict(ref_parts, o=ref_parts["o"][at])
    want_amp = dict(amp, o=amp["o"][at])
    rep.parts(f"{where} fused", got, want, want_amp, R.U_BF16, R.C_BF16)
    rep.lse(f"{where} fused", lse.t.flatten(), ref_lse, lse_amp, False)
    out_s, lse_s, dq_s, dkv_s = _pooled(True, qkv, dout, idx, cu, nseq, L, max_len, H, hd, causal)
    rep.guards(f"{where} split", out_s, lse_s, dq_s, dkv_s)
    got_s = {"o": out_s.t, "dq": dq_s.t, "dk": dkv_s.t[:, :d], "dv": dkv_s.t[:, d:]}
    rep.parts(f"{where} split", got_s, dict(want, dq=ref_parts["dq"][at]), dict(want_amp, dq=amp["dq"][at]), R.U_BF16, R.C_BF16)
    rep.lse(f"{where} split", lse_s.t.flatten(), ref_lse, lse_amp, False)
    same = (torch.equal(out_s.t, out.t) and torch.equal(lse_s.t, lse.t) and torch.equal(dq_s.t, dqkv.t[at, :d])
            and torch.equal(dkv_s.t, dqkv.t[:, d:]))
    rep.expect(where, same, "split and fused results differ in some bit")


# launch_pooled() (csrc/attention_pooled.hip): the 4-rows-per-lane-group instantiation up to 128 rows at head dim 64 (64 at
# head dim 80), the 20-row one up to 640 (320), nothing beyond: clipx_attention_pooled_supported.
@pytest.mark.parametrize("hd,L", [(hd, L) for hd, lengths in R.POOLED_CASES for L in lengths])
def test_pooled_entry_points_dense(hd, L):
    assert ops.attention_pooled_supported(torch.bfloat16, L, hd)
    assert not ops.attention_pooled_supported(torch.bfloat16, {64: 641, 80: 321}[hd], hd)
    rep = Report(f"pooled dense hd{hd} L{L}")
    for kind, causal in R.POOLED_ROWS:
        rows = R.pooled_rows(L, kind)
        idx = (torch.arange(B) * L + rows).to(torch.int32).to(DEV)
        for make in R.FAMILIES:
            qkv = _dev(make(B, L, H, hd)[0], torch.bfloat16)
            dout = _dev(R.pooled_dout(B, H, hd), torch.bfloat16)
            ref = R.reference(qkv, dout, B, L, H, causal, rows=rows)
            pick = (torch.arange(B, device=DEV).repeat_interleave(H) * H + torch.arange(H, device=DEV).repeat(B),
                    rows.to(DEV).repeat_interleave(H))
            _pooled_case(rep, f"{make.__name__} {kind} causal={int(causal)}", qkv, dout, idx, None, B, L, L, hd, causal,
                         ref.parts, ref.amp, ref.lse[pick], ref.lse_amp[pick])
    rep.finish()


@pytest.mark.parametrize("hd,L", [(hd, L) for hd, lengths in R.POOLED_CASES for L in lengths])
def test_pooled_entry_points_packed(hd, L):
    """sequences of L, 1, min(17, L) and a seeded number of rows back to back (cu_rows), max_len = L"""
    g = torch.Generator().manual_seed(100 + L)
    lens = [L, 1, min(17, L), int(torch.randint(1, L + 1, (1,), generator=g))]
    cu = [0]
    for n in lens:
        cu.append(cu[-1] + n)
    nseq, total = len(lens), cu[-1]
    cu_dev = torch.tensor(cu, dtype=torch.int32, device=DEV)
    rep = Report(f"pooled packed hd{hd} L{L}")
    for kind, causal in R.POOLED_ROWS:
        rows = torch.tensor([0 if kind == "first" else n - 1 if kind == "last" else int(torch.randint(0, n, (1,), generator=g))
                             for n in lens])
        idx = (torch.tensor(cu[:-1]) + rows).to(torch.int32).to(DEV)
        for make in R.FAMILIES:
            qkv = _dev(make(1, total, H, hd)[0], torch.bfloat16)
            dout = _dev(R.pooled_dout(nseq, H, hd), torch.bfloat16)
            ref_parts, amp = R.packed_reference(qkv, dout, cu, H, causal, rows=rows)
            ref_lse = torch.empty(nseq * H, dtype=torch.float64, device=DEV)
            lse_amp = torch.empty(nseq * H, dtype=torch.float64, device=DEV)
            for s, n in enumerate(lens):                                   # the pooled rows' log-sum-exp, sequence by sequence
                r = R.reference(qkv[cu[s]:cu[s + 1]], dout[s:s + 1], 1, n, H, causal, rows=rows[s:s + 1])
                ref_lse[s * H:(s + 1) * H] = r.lse[:, int(rows[s])]
                lse_amp[s * H:(s + 1) * H] = r.lse_amp[:, int(rows[s])]
            _pooled_case(rep, f"{make.__name__} {kind} causal={int(causal)}", qkv, dout, idx, cu_dev, nseq, L, L, hd, causal,
                         ref_parts, amp, ref_lse, lse_amp)
    rep.finish()
