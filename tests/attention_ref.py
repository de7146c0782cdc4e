"""Test helper for the attention kernels (csrc/attention.hip, csrc/attention_pooled.hip): an fp64 reference of the forward
and backward, a bound for every ELEMENT of the result, the input families the tests run on, the table of shapes, and a list
of subtly wrong results ("mutations") that the bound has to reject.  torch only, on the CPU or on the tensors' device.  It
lives with the tests because the product has no CPU path.

Reference (per sample and head, hd = head dim, fp64 on the kernel's own -- already rounded -- inputs):

    S = q k^T hd^-1/2 (masked)    P = softmax S    O = P v                      lse = log2 sum_j 2^(S_j log2 e)
    dP = dO v^T    delta = rowsum(P o dP)    dS = P o (dP - delta)
    dQ = hd^-1/2 dS k    dK = hd^-1/2 dS^T q    dV = P^T dO

Bound.  Every element gets its own amplification: the same formulas on absolute values, which is the standard componentwise
bound |fl(A B) - A B| <= gamma |A| |B| carried through the chain:

    A_O = P |v|    A_dV = P^T |dO|    A_delta = rowsum(|dO| o A_O)
    A_dS = P o (|dP| + |delta| + A_delta)    A_dQ = hd^-1/2 A_dS |k|    A_dK = hd^-1/2 A_dS^T |q|

and an element passes when |got - ref| <= C * u * A, with u the unit roundoff of the storage type (2^-8 for bf16, 2^-24
for fp32).  An element whose amplification is exactly 0 (a masked-out row, a key behind a pooled causal row, a filler
sequence with zero dO) must be exactly 0.  The roundings the kernels make at the storage precision are covered term by
term: P and dS rounded to bf16 before they enter an MFMA (u P |v|, u P |dO|, u |dS| <= u A_dS), the outputs rounded to
bf16 (|O| <= A_O, |dV| <= A_dV, |dQ| <= A_dQ, |dK| <= A_dK), delta taken from rowsum(dO o O_bf16) by the backward that is
handed (out, lse) (u |dO| A_O = u A_delta).

One term had to be added to that model, because every kernel rounds where it has none: the scores are fp32 whatever the
storage type, and the exponential turns their ABSOLUTE error into a RELATIVE error of P.  In units of 2^-24 a probability
is off by about

    t_ij = hd^-1/2 |q_i| . |k_j|  +  |S_ij|  +  sum_j P_ij hd^-1/2 |q_i| . |k_j|  +  |ln sum_j e^S_ij|  +  1

(the fp32 dot product; its product with log2 e; the log-sum-exp it is normalised by, which averages the score errors and is
kept -- in LDS, or in memory between forward and backward -- as one fp32 number of its own magnitude), so P + T with
T = (2^-24 / u) P o t stands where P carries a rounding: A_O = (P + T) |v|, A_dV = (P + T)^T |dO|, and A_dS gains
T o |dP - delta|.  In bf16 the term is 2^-16 of the rest and changes nothing; in fp32 it is most of the error wherever |S|
is large: q = -26, k = 1 at head dim 64 puts every score at -208, P is then good to about 208 units and no better, and the
fp32 kernels' dV measured 120 .. 147 against the model without the term and 2 .. 5 against the model with it.

The log-sum-exp (log2 domain, as the kernels store it) is held to C_F32 * 2^-24 * A_lse with

    A_lse = log2 e * sum_j P_j (hd^-1/2 |q| . |k_j|)  +  |lse|  +  1

(first order: d lse = log2 e * sum_j P_j dS_j; the fp32 product S * log2 e and the final m + log2 l round at the size of
lse; exp2 / log2 / the sum are good to a few 2^-24 absolute, the "+ 1").  The online-softmax kernels take l from an MFMA of
ones with the bf16-rounded P: see lse_unit.

Input families (FAMILIES; seeded, every value representable in bf16): random(1), random(3) -- the inputs of
tests/test_kernels_gpu.py --, diagonal(gain), uniform_low, and hot_keys, which is there because the first four cancel so
thoroughly inside dQ and dK that "last 16-row query tile of dQ x0.9" reached 2.9 .. 8.2 on them: below twice any constant the
kernels can meet.  On hot_keys it reaches 14.1 .. 15.9.

Constants.  Never tuned to let a kernel pass: twice the largest ratio measured on the MI355X, rounded up, and capped by the
mutation table (tests/test_attention_bound_cpu.py): every entry of MUTATIONS must reach 2 C_BF16 on some family at each of
MUTATION_SHAPES.  The weakest there: "last key missing from the dQ sum" 12.1 (L = 608 causal, diagonal(4)) and "last
16-row query tile of dQ x0.9" 14.1 (L = 257, head dim 80, hot_keys), so C_BF16 <= 6.  The one exception is "one head's dK
x1.05": a 5 % error cannot exceed 0.05 / 2^-8 = 12.8 even on an element that equals its amplification; it reaches 7.0 .. 8.1
(hot_keys) and has to be rejected at C_BF16 itself, a margin of 1.75.  In 2^-24 units, where the score term
widens the amplification, every mutation still reaches more than 10^4 against 2 C_F32 = 20.

    largest ratio, by part                    o      dq     dk     dv     lse
    CPU emulation, bf16 rounding points       1.86   1.25   1.01   1.97
    CPU emulation, fp32 arithmetic            1.86   1.32   1.27   3.99
    MI355X bf16 whole-sequence (dense)        1.58   1.03   0.83   1.84
    MI355X bf16 whole-sequence (packed)       1.81   1.28   1.08   1.93
    MI355X bf16 online softmax, head dim 64   1.40   1.13   0.97   1.98   0.41 (of C_BF16's unit)
    MI355X bf16 online softmax, head dim 80   1.44   0.94   0.95   1.92   0.37 (of C_BF16's unit)
    MI355X bf16 generic tiled                 0.99   0.70   0.65   1.00
    MI355X bf16 pooled row (fused = split)    0.98   0.39   0.55   1.00   1.99
    MI355X fp32 whole-sequence (dense)        2.01   1.97   1.45   3.20
    MI355X fp32 whole-sequence (packed)       1.79   1.87   2.13   3.58
    MI355X fp32 generic tiled                 2.93   2.20   2.40   4.98

    C_BF16 = 4 = ceil(2 * 1.98)        C_F32 = 10 = ceil(2 * 4.98)
"""
import math

import torch

U_BF16 = 2.0 ** -8
U_F32 = 2.0 ** -24
LOG2E = 1.4426950408889634

BATCH, HEADS = 2, 3
PARTS = ("o", "dq", "dk", "dv")


def unit(dtype) -> float:
    return U_BF16 if dtype == torch.bfloat16 else U_F32


# ---------------------------------------------------------------------------------------------------------- layout
def split_heads(x, batch, L, heads):
    """[batch*L, heads*hd] -> [batch, heads, L, hd]"""
    return x.reshape(batch, L, heads, -1).permute(0, 2, 1, 3)


def merge_heads(x):
    """[batch, heads, L, hd] -> [batch*L, heads*hd]"""
    b, h, L, hd = x.shape
    return x.permute(0, 2, 1, 3).reshape(b * L, h * hd)


def split_qkv(qkv, batch, L, heads):
    d = qkv.shape[-1] // 3
    return tuple(split_heads(qkv[:, i * d:(i + 1) * d], batch, L, heads) for i in range(3))


def parts_of(out, dqkv):
    """the kernels' two result buffers (out [rows, d], dqkv [rows, 3 d]) as the four parts"""
    d = out.shape[-1]
    return {"o": out, "dq": dqkv[:, :d], "dk": dqkv[:, d:2 * d], "dv": dqkv[:, 2 * d:]}


def scatter_rows(dout_rows, rows, batch, L):
    """dO of the pooled rows ([batch, d], position rows[s] of sequence s) as a full [batch*L, d] with zeros elsewhere"""
    full = torch.zeros(batch * L, dout_rows.shape[-1], dtype=dout_rows.dtype, device=dout_rows.device)
    full[torch.arange(batch, device=dout_rows.device) * L + rows.to(dout_rows.device).long()] = dout_rows
    return full


# ---------------------------------------------------------------------------------------------------------- reference
class Ref:
    """parts / amp: {"o", "dq", "dk", "dv"} -> [batch*L, d] fp64; lse / lse_amp [batch*heads, L]; the intermediates
    (q, k, v, do, P, dP, delta, dS: [batch, heads, L, .]) are kept for the mutations."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def _mask(L, device, admit=0):
    """True where key j is hidden from query i (j > i + admit)"""
    return torch.ones(L, L, dtype=torch.bool, device=device).triu(1 + admit)


def reference(qkv, dout, batch, L, heads, causal, rows=None, u=None, _admit=0, _delta_shift=0):
    """The fp64 reference and every element's amplification.  qkv [batch*L, 3 d] (q | k | v per row), dout [batch*L, d],
    or [batch, d] with rows [batch] (positions inside the sequences): the gradient of the pooled rows alone.  u: the unit
    the amplification will be multiplied by (default: that of qkv's dtype); it only weighs the fp32 score term.
    _admit / _delta_shift exist for MUTATIONS (a mask that lets key i + 1 through, delta read from the neighbouring head)."""
    kappa = U_F32 / (unit(qkv.dtype) if u is None else u)
    if rows is not None:
        dout = scatter_rows(dout, rows, batch, L)
    q, k, v = split_qkv(qkv.double(), batch, L, heads)
    do = split_heads(dout.double(), batch, L, heads)
    hd = q.shape[-1]
    sc = hd ** -0.5
    S = q @ k.transpose(-1, -2) * sc
    AS = q.abs() @ k.abs().transpose(-1, -2) * sc
    if causal:
        S = S.masked_fill(_mask(L, S.device, _admit), float("-inf"))
    m = S.max(-1, keepdim=True).values
    E = torch.exp(S - m)
    l = E.sum(-1, keepdim=True)
    P = E / l
    lse = (m + torch.log(l)).squeeze(-1) * LOG2E
    O = P @ v
    dP = do @ v.transpose(-1, -2)
    delta = (P * dP).sum(-1, keepdim=True)
    if _delta_shift:
        delta = delta.roll(_delta_shift, 1)
    dS = P * (dP - delta)
    dQ = dS @ k * sc
    dK = dS.transpose(-1, -2) @ q * sc
    dV = P.transpose(-1, -2) @ do
    # relative error of P in units of 2^-24: the fp32 dot product, its product with log2 e, and the log-sum-exp it is
    # normalised by (itself a P-weighted mean of score errors, stored in fp32 at its own magnitude)
    T = kappa * P * (AS + S.abs().masked_fill(P == 0, 0.0) + (P * AS).sum(-1, keepdim=True) + (m + torch.log(l)).abs() + 1.0)
    A_O = (P + T) @ v.abs()
    A_dV = (P + T).transpose(-1, -2) @ do.abs()
    A_delta = (do.abs() * A_O).sum(-1, keepdim=True)
    A_dS = P * (dP.abs() + delta.abs() + A_delta) + T * (dP - delta).abs()
    A_dQ = A_dS @ k.abs() * sc
    A_dK = A_dS.transpose(-1, -2) @ q.abs() * sc
    lse_amp = LOG2E * (P * AS).sum(-1) + lse.abs() + 1.0
    return Ref(batch=batch, L=L, heads=heads, hd=hd, causal=causal,
               parts={"o": merge_heads(O), "dq": merge_heads(dQ), "dk": merge_heads(dK), "dv": merge_heads(dV)},
               amp={"o": merge_heads(A_O), "dq": merge_heads(A_dQ), "dk": merge_heads(A_dK), "dv": merge_heads(A_dV)},
               lse=lse.reshape(batch * heads, L), lse_amp=lse_amp.reshape(batch * heads, L),
               q=q, k=k, v=v, do=do, P=P, dP=dP, delta=delta, dS=dS)


def packed_reference(qkv, dout, cu, heads, causal, rows=None):
    """The same for sequences of different lengths stored back to back (rows cu[s] .. cu[s+1] of qkv): every sequence
    against the reference of that sequence alone (sequences of equal length share one call).  dout [total, d], or [nseq, d]
    with rows [nseq] (positions inside the sequences).  Returns (parts, amp) in the packed layout."""
    d = qkv.shape[-1] // 3
    nseq, total = len(cu) - 1, cu[-1]
    parts = {p: torch.zeros(total, d, dtype=torch.float64, device=qkv.device) for p in PARTS}
    amp = {p: torch.zeros(total, d, dtype=torch.float64, device=qkv.device) for p in PARTS}
    by_len = {}
    for s in range(nseq):
        by_len.setdefault(cu[s + 1] - cu[s], []).append(s)
    for n, seqs in by_len.items():
        at = (torch.tensor([cu[s] for s in seqs], device=qkv.device).unsqueeze(1)
              + torch.arange(n, device=qkv.device).unsqueeze(0)).reshape(-1)
        if rows is None:
            r = reference(qkv[at], dout[at], len(seqs), n, heads, causal)
        else:
            sel = torch.tensor(seqs, device=qkv.device)
            r = reference(qkv[at], dout[sel], len(seqs), n, heads, causal, rows=rows.to(qkv.device)[sel])
        for p in PARTS:
            parts[p][at] = r.parts[p]
            amp[p][at] = r.amp[p]
    return parts, amp


# ---------------------------------------------------------------------------------------------------------- the measure
def ratio(got, ref, amp, u) -> float:
    """max over elements of |got - ref| / (u amp); inf when an element of zero amplification is not exactly zero (or when
    anything is not finite)."""
    got = got.double()
    if got.numel() == 0:
        return 0.0
    if not bool(torch.isfinite(got).all()):
        return math.inf
    err = (got - ref).abs()
    zero = amp == 0
    if bool((err[zero] != 0).any()):
        return math.inf
    return float((err / (u * amp).masked_fill(zero, 1.0)).max())


def ratios(got, ref, amp, u):
    """{part: ratio} for dicts of the four parts (any subset of got's keys)"""
    return {p: ratio(got[p], ref[p], amp[p], u) for p in got}


def lse_unit(lse_amp, sums_rounded_p):
    """(unit, constant) of the log-sum-exp check: |lse - ref| <= constant * unit.  fp32 sums (the pooled-row kernels):
    2^-24 A_lse under C_F32.  The online-softmax kernels take the row sum l from an MFMA of ones with the bf16-rounded
    probabilities, the same P that multiplies V: each term is off by at most 2^-8 of itself, so l by 2^-8 l and the
    log-sum-exp by 2^-8 log2 e, under C_BF16, on top of the fp32 part."""
    if sums_rounded_p:
        return U_BF16 * LOG2E + (C_F32 / C_BF16) * U_F32 * lse_amp, C_BF16
    return U_F32 * lse_amp, C_F32


def relerr(a, b) -> float:
    """the measure of tests/test_kernels_gpu.py: one scalar, every element's error against the largest entry"""
    return float((a.double() - b.double()).abs().max() / (b.double().abs().max() + 1e-12))


# ---------------------------------------------------------------------------------------------------------- inputs
def _bf16_values(x):
    return x.to(torch.bfloat16).float()


def _randn(shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def random(scale):
    """the inputs of tests/test_kernels_gpu.py: qkv ~ scale N(0, 1) (seed 1), dO ~ N(0, 1) (seed 2)"""
    def make(batch, L, heads, hd):
        d = heads * hd
        return _bf16_values(_randn((batch * L, 3 * d), 1) * scale), _bf16_values(_randn((batch * L, d), 2))
    make.__name__ = f"random({scale:g})"
    return make


def diagonal(gain):
    """q_i = gain k_i / sqrt(hd) + 0.3 noise: the score of query i with its own key is about gain |k_i|^2 / hd ~ gain above
    the rest, so a dropped or mis-masked key ruins the row it belongs to"""
    def make(batch, L, heads, hd):
        d = heads * hd
        k = _randn((batch * L, d), 11)
        q = gain * k * hd ** -0.5 + 0.3 * _randn((batch * L, d), 12)
        v = _randn((batch * L, d), 13)
        return _bf16_values(torch.cat([q, k, v], 1)), _bf16_values(_randn((batch * L, d), 2))
    make.__name__ = f"diagonal({gain:g})"
    return make


def uniform_low(batch, L, heads, hd):
    """q = -26, k = 1: every score is far below zero (log-sum-exp about -300 in the log2 domain at head dim 64) and the
    attention is uniform, so a key that is padding inside the kernel would outweigh every real one"""
    d = heads * hd
    qkv = torch.cat([torch.full((batch * L, d), -26.0), torch.ones(batch * L, d), _randn((batch * L, d), 5)], 1)
    return _bf16_values(qkv), _bf16_values(_randn((batch * L, d), 2))


def hot_keys(batch, L, heads, hd):
    """One key in HOT_EVERY carries the values: v large and positive there and near zero elsewhere, k positive there and small
    elsewhere, q and dO positive.  dP is then large on the hot keys only, delta and its amplification stay a fraction of it,
    and the sums that make dQ and dK add terms of one sign: the elements are close to their own amplification, so a tile
    or a head that is off by a few per cent shows at nearly its full relative size instead of drowning in cancellation."""
    d = heads * hd
    hot = (torch.arange(batch * L) % L % HOT_EVERY == 0).unsqueeze(1)
    k = torch.where(hot, 1.0 + 0.1 * _randn((batch * L, d), 21), 0.1 * _randn((batch * L, d), 22))
    v = torch.where(hot, 4.0 * _randn((batch * L, d), 23).abs(), 0.05 * _randn((batch * L, d), 24))
    q = 0.3 * _randn((batch * L, d), 25).abs()
    return _bf16_values(torch.cat([q, k, v], 1)), _bf16_values(_randn((batch * L, d), 2).abs())


HOT_EVERY = 32
DIAGONAL_GAIN = 4.0
FAMILIES = (random(1.0), random(3.0), diagonal(DIAGONAL_GAIN), uniform_low, hot_keys)


def pooled_dout(batch, heads, hd):
    return _bf16_values(_randn((batch, heads * hd), 2))


def pooled_rows(L, kind, batch=BATCH):
    """positions of the pooled rows: "first", "last" or seeded random"""
    if kind == "first":
        return torch.zeros(batch, dtype=torch.long)
    if kind == "last":
        return torch.full((batch,), L - 1, dtype=torch.long)
    return torch.randint(0, L, (batch,), generator=torch.Generator().manual_seed(L))


# ---------------------------------------------------------------------------------------------------------- shapes
# (group, dtype, head dim, lengths, causal values): the dense entry points; batch BATCH, heads HEADS throughout
DENSE_CASES = (
    ("f32_whole", torch.float32, 32, (1, 5, 17, 64, 77, 128), (False, True)),
    ("f32_whole", torch.float32, 64, (1, 5, 17, 64, 77, 128), (False, True)),
    ("f32_whole", torch.float32, 80, (1, 5, 17, 64, 77, 128), (False, True)),
    ("bf16_whole", torch.bfloat16, 64, (16, 17, 32, 33, 64, 65, 96, 97, 127, 128), (False, True)),
    ("bf16_online64", torch.bfloat16, 64, (129, 130, 225, 320, 321, 607, 608), (False, True)),
    ("bf16_online80", torch.bfloat16, 80, (33, 257, 287, 288), (False, True)),
    ("bf16_generic", torch.bfloat16, 64, (609,), (False, True)),
    ("bf16_generic", torch.bfloat16, 80, (289,), (False, True)),
    ("bf16_generic", torch.bfloat16, 128, (130,), (False, True)),
    ("bf16_generic", torch.bfloat16, 32, (50,), (False, True)),
    ("f32_generic", torch.float32, 128, (130,), (False, True)),
    ("f32_generic", torch.float32, 64, (700,), (True,)),
)
ONLINE_GROUPS = ("bf16_online64", "bf16_online80")       # the shapes with a log-sum-exp hand-over
# (head dim, lengths): the pooled-row kernels; each length on both sides of the short / long instantiation and the last
POOLED_CASES = ((64, (50, 128, 129, 640)), (80, (33, 64, 65, 320)))
# (pooled-row kind, causal)
POOLED_ROWS = (("first", False), ("first", True), ("last", True), ("random", True))


def dense_cases():
    for group, dtype, hd, lengths, causals in DENSE_CASES:
        for L in lengths:
            for causal in causals:
                yield group, dtype, hd, L, causal


# ---------------------------------------------------------------------------------------------------------- emulation
def _r16(x):
    return x.to(torch.bfloat16).float()


def emulate_bf16(qkv, dout, batch, L, heads, causal, delta_from_out=False, rows=None):
    """The bf16 kernels' rounding points in plain fp32 torch: S and every sum in fp32, P rounded to bf16 before P v and
    P^T dO, dS rounded to bf16, outputs rounded to bf16; delta from rowsum(P o dP) (two-sweep backward) or from
    rowsum(dO o O_bf16) (the backward that is handed out and lse).  Returns the four parts."""
    if rows is not None:
        dout = scatter_rows(dout, rows, batch, L)
    q, k, v = split_qkv(qkv.float(), batch, L, heads)
    do = split_heads(dout.float(), batch, L, heads)
    sc = q.shape[-1] ** -0.5
    S = q @ k.transpose(-1, -2) * sc
    if causal:
        S = S.masked_fill(_mask(L, S.device), float("-inf"))
    P = torch.softmax(S, -1)
    P16 = _r16(P)
    O = _r16(P16 @ v)
    dP = do @ v.transpose(-1, -2)
    delta = (do * O).sum(-1, keepdim=True) if delta_from_out else (P * dP).sum(-1, keepdim=True)
    dS = _r16(P * (dP - delta))
    return {"o": merge_heads(O), "dq": merge_heads(_r16(dS @ k * sc)),
            "dk": merge_heads(_r16(dS.transpose(-1, -2) @ q * sc)), "dv": merge_heads(_r16(P16.transpose(-1, -2) @ do))}


def emulate_f32(qkv, dout, batch, L, heads, causal):
    """the reference's formulas in fp32 arithmetic: what an fp32 kernel may differ by from fp64"""
    q, k, v = split_qkv(qkv.float(), batch, L, heads)
    do = split_heads(dout.float(), batch, L, heads)
    sc = q.shape[-1] ** -0.5
    S = q @ k.transpose(-1, -2) * sc
    if causal:
        S = S.masked_fill(_mask(L, S.device), float("-inf"))
    P = torch.softmax(S, -1)
    dP = do @ v.transpose(-1, -2)
    dS = P * (dP - (P * dP).sum(-1, keepdim=True))
    return {"o": merge_heads(P @ v), "dq": merge_heads(dS @ k * sc), "dk": merge_heads(dS.transpose(-1, -2) @ q * sc),
            "dv": merge_heads(P.transpose(-1, -2) @ do)}


# ---------------------------------------------------------------------------------------------------------- mutations
# Each takes (ref, qkv, dout) and returns the four parts of a result that is wrong in the way its name says.
def _clone(r):
    return {p: t.clone() for p, t in r.parts.items()}


def _rows_at(r, pos):
    """rows of the [batch*L, d] layout that hold position pos of every sequence"""
    return torch.arange(r.batch, device=r.P.device) * r.L + pos


def mut_last_key_dkdv_zero(r, qkv, dout):
    out = _clone(r)
    out["dk"][_rows_at(r, r.L - 1)] = 0
    out["dv"][_rows_at(r, r.L - 1)] = 0
    return out


def mut_last_key_missing_from_dq(r, qkv, dout):
    out = _clone(r)
    out["dq"] -= merge_heads(r.dS[..., -1:] * r.k[..., -1:, :] * r.hd ** -0.5)
    return out


def mut_last_query_misses_last_key(r, qkv, dout):
    out = _clone(r)
    O = r.P[..., -1:, -1:] * r.v[..., -1:, :]                              # [batch, heads, 1, hd]: the term that is lost
    out["o"][_rows_at(r, r.L - 1)] -= O.permute(0, 2, 1, 3).reshape(r.batch, -1)
    return out


def mut_mask_admits_next_key(r, qkv, dout):
    """(only defined under a causal mask: the mutation table runs it with causal = True at every shape)"""
    return reference(qkv, dout, r.batch, r.L, r.heads, True, _admit=1).parts


def mut_last_query_tile_dq_scaled(r, qkv, dout):
    out = _clone(r)
    t0 = (r.L - 1) // 16 * 16
    at = (torch.arange(r.batch, device=r.P.device).unsqueeze(1) * r.L + torch.arange(t0, r.L, device=r.P.device)).reshape(-1)
    out["dq"][at] *= 0.9
    return out


def mut_one_head_dk_scaled(r, qkv, dout):
    out = _clone(r)
    out["dk"][:, r.hd:2 * r.hd] *= 1.05
    return out


def mut_heads_swapped(r, qkv, dout):
    out = _clone(r)
    for p in PARTS:
        out[p][:, :r.hd] = r.parts[p][:, r.hd:2 * r.hd]
        out[p][:, r.hd:2 * r.hd] = r.parts[p][:, :r.hd]
    return out


def mut_delta_from_wrong_head(r, qkv, dout):
    return reference(qkv, dout, r.batch, r.L, r.heads, r.causal, _delta_shift=1).parts


MUTATIONS = (
    ("last key row of dK/dV zero", mut_last_key_dkdv_zero),
    ("last key missing from the dQ sum", mut_last_key_missing_from_dq),
    ("last query row of O missing its last key", mut_last_query_misses_last_key),
    ("causal mask admitting key i+1", mut_mask_admits_next_key),
    ("last 16-row query tile of dQ x0.9", mut_last_query_tile_dq_scaled),
    ("one head's dK x1.05", mut_one_head_dk_scaled),
    ("one head swapped with its neighbour", mut_heads_swapped),
    ("delta taken from the wrong head", mut_delta_from_wrong_head),
)
WEAK_MUTATION = "one head's dK x1.05"          # held to C_BF16, not 2 C_BF16: see the module docstring
# (L, head dim, causal) at which every mutation must be rejected on at least one family
MUTATION_SHAPES = ((77, 64, True), (608, 64, True), (197, 64, False), (257, 80, False))

# ---------------------------------------------------------------------------------------------------------- constants
# the measurements and the cap behind these two are in the module docstring
C_BF16 = 4.0
C_F32 = 10.0
