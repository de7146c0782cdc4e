"""CPU-side checks of the fused MaxSim below 64 image tokens per image (ViT-B-32-colxlip: 49): the model config, and the sizes
of the partial arrays -- per (row, image, slot half) for 16 <= q < 64, per (row, 64-column slot, segment) above, as
csrc/gemm_nt_maxsim.h writes them."""
import pytest
import torch

from colxlip_amd import create_model_and_transforms, get_model_config, ops
from tests.late_interaction_ref import cu_of as _cu, packed_counts as _counts
from tests.test_late_interaction_cpu import GIB2, PLAN_GRID

SMALL_Q = (16, 17, 24, 49, 63)


def test_b32_colxlip_config_and_parameter_schema():
    """ViT-B-32-colxlip (named by the reference's launch line, src/colxlip.sh:38) is ViT-B-16-colxlip with 32-pixel patches: the
    same parameter names, and only the patch embedding and the positional embedding (50 instead of 197 rows) differ in shape."""
    c32, c16 = get_model_config("ViT-B-32-colxlip"), get_model_config("ViT-B-16-colxlip")
    assert c32 is not None and c32["vision_cfg"]["patch_size"] == 32
    c32["vision_cfg"]["patch_size"] = 16
    assert c32 == c16
    shapes = {}
    for name in ("ViT-B-32-colxlip", "ViT-B-16-colxlip"):
        model, _, _ = create_model_and_transforms(name, precision="fp32", device="cpu", output_dict=True)
        assert type(model).__name__ == "ColXLIP"
        shapes[name] = {k: tuple(p.shape) for k, p in model.named_parameters()}
        del model
    a, b = shapes["ViT-B-32-colxlip"], shapes["ViT-B-16-colxlip"]
    assert sorted(a) == sorted(b)
    assert sorted(k for k in a if a[k] != b[k]) == ["visual.conv1.weight", "visual.positional_embedding"]
    assert a["visual.conv1.weight"] == (768, 3, 32, 32) and a["visual.positional_embedding"] == (50, 768)


@pytest.mark.parametrize("q", SMALL_Q)
def test_partial_bytes_below_64_tokens(q):
    """6 bytes per (row, image, slot half): an image of fewer than 64 tokens lies in at most two 64-column slots"""
    for ci in (1, 8, 512):
        for rows in (1, 16, 17, 4096):
            ld = ops.maxsim_partial_ld(rows)
            assert ld >= rows and ld % 16 == 0
            assert ops.maxsim_partial_rows(ci, q) == 2 * ci
            assert ops.maxsim_partial_bytes(ci, q, rows) == 12 * ci * ld
            # every (image, half) the epilogue can write has a row: image k begins in slot (k q) >> 6 (half 0) and may end in
            # the next one (half 1), never further
            for k in range(ci):
                assert ((k + 1) * q - 1) // 64 - (k * q) // 64 <= 1


@pytest.mark.parametrize("ni,q,e,counts,partial_bytes,operand_bytes", PLAN_GRID)
def test_partial_bytes_from_64_tokens_are_unchanged(ni, q, e, counts, partial_bytes, operand_bytes):
    assert q >= 64
    for ci in (1, ni, (ni + 7) // 8 * 8):
        for rows in (1, 16, 100, sum(counts)):
            slots = (ci * q + 63) // 64
            assert ops.maxsim_partial_rows(ci, q) == 2 * slots
            assert ops.maxsim_partial_bytes(ci, q, rows) == 12 * slots * ops.maxsim_partial_ld(rows)


SMALL_PLAN_GRID = [(ni, q, e, counts, pb, ob) for q in SMALL_Q for ni, e, counts, pb, ob in [
    (5, 128, _counts(7, 20, 0), 2 << 30, None),
    (20, 128, _counts(7, 20, 1), 12 * 8 * 16, 8 * q * 128 * 2),         # 8 images per chunk (a multiple of every alignment unit), 16 rows
    (512, 512, _counts(512, 77, 4), 2 << 30, None),                     # the training shape: one chunk each
    (5000, 512, _counts(25000, 77, 5), 2 << 30, None),                  # COCO 5k
    (70000, 128, _counts(300, 30, 7), 8 << 30, 64 << 30),               # more than 65535 images
    (40, 1024, _counts(50, 77, 8), 1 << 18, None),                      # small partial limit: the image chunk shrinks
    (9, 128, [300, 4, 500, 7], 12 * 16 * 32, None),                     # samples larger than a text chunk stand alone
]]


@pytest.mark.parametrize("ni,q,e,counts,partial_bytes,operand_bytes", SMALL_PLAN_GRID)
def test_chunk_plan_below_64_tokens(ni, q, e, counts, partial_bytes, operand_bytes):
    """tests/test_late_interaction_cpu.py::test_chunk_plan's invariants, and the arrays `_maxsim_scores_fused` allocates hold what
    the kernels of every (image chunk, text chunk) write"""
    cu = _cu(counts)
    nt = len(counts)
    image_chunks, text_chunks = ops.plan_maxsim_chunks(ni, q, e, cu, partial_bytes, operand_bytes)
    limit = GIB2 if operand_bytes is None else operand_bytes
    assert image_chunks[0][0] == 0 and image_chunks[-1][1] == ni
    for (k0, k1, ci), nxt in zip(image_chunks, image_chunks[1:] + [None]):
        assert k0 < k1 <= ni and ci >= k1 - k0
        assert (ci * q) % 8 == 0 and ci <= 65535
        assert ci * q * e * 2 <= limit
        if nxt is not None:
            assert nxt[0] == k1 and ci == k1 - k0
        else:
            assert ci - (k1 - k0) < 8
    assert text_chunks[0][0] == 0 and text_chunks[-1][1] == nt
    cmax = max(ci for _, _, ci in image_chunks)
    for (m0, m1, r0, r1), nxt in zip(text_chunks, text_chunks[1:] + [None]):
        assert m0 < m1 <= nt and (r0, r1) == (cu[m0], cu[m1])
        if nxt is not None:
            assert nxt[0] == m1
        if m1 - m0 > 1:
            assert ops.maxsim_partial_bytes(cmax, q, r1 - r0) <= partial_bytes
    # the allocation of _maxsim_scores_fused: [partial rows of the largest image chunk, largest ld]
    ldmax = ops.maxsim_partial_ld(max(r1 - r0 for _, _, r0, r1 in text_chunks))
    alloc = ops.maxsim_partial_rows(cmax, q) * ldmax
    for _, _, ci in image_chunks:
        for _, _, r0, r1 in text_chunks:
            ldp = ops.maxsim_partial_ld(r1 - r0)
            assert ldp >= r1 - r0
            assert (2 * (ci - 1) + 1) * ldp + (r1 - r0) <= alloc        # the last element the GEMM epilogue can write
            assert 6 * alloc >= ops.maxsim_partial_bytes(ci, q, r1 - r0)


@pytest.mark.parametrize("q", SMALL_Q + (64, 196))
def test_loss_forward_allocation_fits_partial_bytes(q, monkeypatch):
    """`_MaxSimFused.forward` sizes pmax / pidx as [maxsim_partial_rows(ni, q), ldp]: what it hands the kernels is never smaller
    than `maxsim_partial_bytes` of the chunk.  Run on the CPU with the four kernel wrappers replaced by recorders."""
    from colxlip_amd import loss as LS
    ni, nt, n, e = 8, 4, 9, 128
    R = 23
    seen = []
    monkeypatch.setattr(ops, "maxsim_pack_text", lambda txt: (torch.zeros(nt + 1, dtype=torch.int32), R))
    monkeypatch.setattr(ops, "maxsim_pack_rows", lambda txt, cu, r: (torch.zeros(r, e), torch.zeros(r, dtype=torch.int32), torch.ones(r)))
    monkeypatch.setattr(ops, "maxsim_gemm", lambda packed, img, ni_, q_, pmax, pidx, ldp: seen.append(
        (packed.shape[0], ni_, q_, tuple(pmax.shape), tuple(pidx.shape), pmax.dtype, pidx.dtype, ldp)))
    monkeypatch.setattr(ops, "maxsim_finish", lambda *a: None)
    monkeypatch.setattr(ops, "maxsim_mean", lambda nt_, ni_, ld, cu, row_w, maxvT: (torch.zeros(nt_, ni_), torch.zeros(nt_, ni_)))

    class Ctx:
        def save_for_backward(self, *a):
            pass

    LS._MaxSimFused.forward(Ctx(), torch.zeros(ni, q, e), torch.zeros(nt, n, e))
    assert len(seen) == 1
    rows, ni_, q_, ps, is_, pd, idt, ldp = seen[0]
    assert (rows, ni_, q_) == (R, ni, q) and ps == is_ and pd == torch.float32 and idt == torch.int16
    assert ps == (ops.maxsim_partial_rows(ni, q), ldp) and ldp >= R
    assert 6 * ps[0] * ps[1] >= ops.maxsim_partial_bytes(ni, q, R)
    assert ps[0] == (2 * ni if q < 64 else 2 * ((ni * q + 63) // 64))
