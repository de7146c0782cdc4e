"""The per-element attention bound of tests/attention_ref.py, proven on the CPU before it judges a kernel:

  * an emulation of the kernels' own rounding points stays inside it at every shape and family of the GPU tests,
  * every entry of MUTATIONS (results that are subtly wrong: a dropped key row, a mask off by one, a head scaled by 5 %)
    is rejected by it, with a factor of two to spare, at each of MUTATION_SHAPES,
  * and the measure it replaces -- max|a - b| / max|b| over the whole tensor -- is shown to accept one of them.
"""
import pytest
import torch

from tests import attention_ref as R

B, H = R.BATCH, R.HEADS


def _inputs(make, L, hd):
    return make(B, L, H, hd)


def _fmt(r):
    return "  ".join(f"{p} {v:.3g}" for p, v in r.items())


@pytest.mark.parametrize("group,dtype,hd", sorted({(g, d, hd) for g, d, hd, _, _ in R.DENSE_CASES}, key=str))
def test_emulated_kernel_rounding_is_accepted(group, dtype, hd):
    """bf16 shapes: the emulation of the kernels' rounding points, with delta from either source; fp32 shapes: fp32
    arithmetic against fp64.  The largest ratios seen are recorded in attention_ref's docstring."""
    worst = {}
    for g, dt, hd_, L, causal in R.dense_cases():
        if (g, dt, hd_) != (group, dtype, hd):
            continue
        for make in R.FAMILIES:
            qkv, dout = _inputs(make, L, hd)
            ref = R.reference(qkv, dout, B, L, H, causal, u=R.unit(dtype))
            if dtype == torch.bfloat16:
                runs = [R.emulate_bf16(qkv, dout, B, L, H, causal, delta_from_out=f) for f in (False, True)]
            else:
                runs = [R.emulate_f32(qkv, dout, B, L, H, causal)]
            for got in runs:
                for p, v in R.ratios(got, ref.parts, ref.amp, R.unit(dtype)).items():
                    worst[p] = max(worst.get(p, 0.0), v)
    print(f"emulation {group} hd {hd}: {_fmt(worst)}")
    assert max(worst.values()) <= (R.C_BF16 if dtype == torch.bfloat16 else R.C_F32), worst


@pytest.mark.parametrize("hd,lengths", R.POOLED_CASES)
def test_emulated_pooled_rounding_is_accepted(hd, lengths):
    """the pooled-row shapes (dO on one row per sequence): the same emulation, and exact zeros where nothing flows"""
    worst = {}
    for L in lengths:
        for kind, causal in R.POOLED_ROWS:
            rows = R.pooled_rows(L, kind)
            for make in R.FAMILIES:
                qkv, _ = _inputs(make, L, hd)
                dout = R.pooled_dout(B, H, hd)
                ref = R.reference(qkv, dout, B, L, H, causal, rows=rows, u=R.U_BF16)
                got = R.emulate_bf16(qkv, dout, B, L, H, causal, rows=rows)
                for p, v in R.ratios(got, ref.parts, ref.amp, R.U_BF16).items():
                    worst[p] = max(worst.get(p, 0.0), v)
                if causal:
                    for s in range(B):
                        behind = slice(s * L + int(rows[s]) + 1, (s + 1) * L)
                        assert float(ref.amp["dk"][behind].abs().max() if int(rows[s]) + 1 < L else 0.0) == 0.0
    print(f"emulation pooled hd {hd}: {_fmt(worst)}")
    assert max(worst.values()) <= R.C_BF16, worst


@pytest.mark.parametrize("L,hd,causal", R.MUTATION_SHAPES)
def test_mutations_are_rejected(L, hd, causal):
    """Every mutation reaches 2 C_BF16 on at least one family (the 5 % head: C_BF16, its ceiling is 12.8; the figures are in
    attention_ref's docstring), and 2 C_F32 in the 2^-24 units an fp32 kernel is held to.  The mask mutation exists only
    under a causal mask, so it runs with causal = True at every shape."""
    refs = {}
    for make in R.FAMILIES:
        qkv, dout = _inputs(make, L, hd)
        refs[make.__name__] = (qkv, dout, {(c, u): R.reference(qkv, dout, B, L, H, c, u=u)
                                           for c in {causal, True} for u in (R.U_BF16, R.U_F32)})
    for name, mutate in R.MUTATIONS:
        c = True if mutate is R.mut_mask_admits_next_key else causal
        for u, need in ((R.U_BF16, R.C_BF16 if name == R.WEAK_MUTATION else 2 * R.C_BF16), (R.U_F32, 2 * R.C_F32)):
            best = {}
            for fam, (qkv, dout, ref_of) in refs.items():
                ref = ref_of[c, u]
                best[fam] = max(R.ratios(mutate(ref, qkv, dout), ref.parts, ref.amp, u).values())
            print(f"mutation L={L} hd={hd} causal={c} u=2^{'-8' if u == R.U_BF16 else '-24'} {name!r}: "
                  + "  ".join(f"{f} {v:.3g}" for f, v in best.items()))
            assert max(best.values()) >= need, (name, u, best)


def test_accepted_results_are_not_rejected_by_construction():
    """the measure itself: the reference against itself is 0, an element of zero amplification that is not zero is inf"""
    qkv, dout = _inputs(R.FAMILIES[0], 17, 64)
    ref = R.reference(qkv, dout, B, 17, H, True, u=R.U_BF16)
    assert max(R.ratios(ref.parts, ref.parts, ref.amp, R.U_BF16).values()) == 0.0
    rows = R.pooled_rows(17, "first")
    refp = R.reference(qkv, R.pooled_dout(B, H, 64), B, 17, H, True, rows=rows, u=R.U_BF16)
    assert float(refp.amp["dv"][1:17].abs().max()) == 0.0               # keys behind the pooled row 0
    bad = {p: t.clone() for p, t in refp.parts.items()}
    bad["dv"][5, 3] = 1e-30
    assert R.ratios(bad, refp.parts, refp.amp, R.U_BF16)["dv"] == float("inf")


def test_old_measure_accepts_a_dropped_key_row():
    """Why this file exists: max|a - b| / max|b| < 3e-2, the bf16 backward bound of tests/test_kernels_gpu.py, accepts dK
    and dV whose last key row is zero (random(1.0), L = 608, causal) -- the ragged last tile, where a kernel is most likely
    to be wrong.  The per-element bound rejects the same result."""
    L, hd = 608, 64
    qkv, dout = _inputs(R.random(1.0), L, hd)
    ref = R.reference(qkv, dout, B, L, H, True, u=R.U_BF16)
    bad = R.mut_last_key_dkdv_zero(ref, qkv, dout)
    cat = lambda p: torch.cat([p["dq"], p["dk"], p["dv"]], 1)       # noqa: E731
    old = R.relerr(cat(bad), cat(ref.parts))
    print(f"old measure on the dropped key row: {old:.4f}")
    assert old < 3e-2
    assert max(R.ratios(bad, ref.parts, ref.amp, R.U_BF16).values()) >= 2 * R.C_BF16
