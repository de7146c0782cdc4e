"""CPU-side checks of late-interaction retrieval: the chunk plan of `ops.maxsim_scores` (a pure function), the
`--evaluate-as-original-clip` flag, and the binding of the new C entry point."""
import ctypes

import pytest

from colxlip_amd import _lib, ops
from colxlip_amd.params import parse_args
from tests.late_interaction_ref import cu_of as _cu, packed_counts as _counts

GIB2 = (1 << 31) - 1


PLAN_GRID = [
    # ni, q, e, packed rows per sample, partial bytes, operand bytes
    (5, 64, 128, _counts(6, 9, 0), 2 << 30, None),
    (5, 100, 256, _counts(7, 7, 1), 2 << 30, None),                     # (5 * 100) % 8 != 0: padded to 6 images
    (5, 100, 256, _counts(7, 7, 1), 12 * 4 * 16, 2 * 100 * 256 * 2),    # 2 images per chunk, 16 rows per text chunk
    (6, 196, 128, _counts(9, 77, 2), 12 * 13 * 96, 4 * 196 * 128 * 2),
    (7, 65, 128, _counts(5, 20, 3), 2 << 30, None),                     # q odd: image counts in multiples of 8
    (512, 196, 512, _counts(512, 77, 4), 2 << 30, None),                # the training shape: one chunk each
    (5000, 196, 512, _counts(25000, 77, 5), 2 << 30, None),             # COCO 5k: one image chunk, the text in chunks
    (30000, 196, 512, _counts(2000, 77, 6), 2 << 30, None),             # the image operand passes 2 GiB
    (70000, 64, 128, _counts(300, 30, 7), 8 << 30, 64 << 30),           # more than 65535 images
    (40, 576, 1024, _counts(50, 77, 8), 1 << 20, None),                 # small partial limit: the image chunk shrinks
    (9, 64, 128, [300, 4, 500, 7], 12 * 9 * 32, None),                  # samples larger than a text chunk stand alone
]


@pytest.mark.parametrize("ni,q,e,counts,partial_bytes,operand_bytes", PLAN_GRID)
def test_chunk_plan(ni, q, e, counts, partial_bytes, operand_bytes):
    cu = _cu(counts)
    nt = len(counts)
    image_chunks, text_chunks = ops.plan_maxsim_chunks(ni, q, e, cu, partial_bytes, operand_bytes)
    limit = GIB2 if operand_bytes is None else operand_bytes
    # every image once, in order; only the last chunk padded; alignment, count and operand size of every chunk
    assert image_chunks[0][0] == 0 and image_chunks[-1][1] == ni
    for (k0, k1, ci), nxt in zip(image_chunks, image_chunks[1:] + [None]):
        assert k0 < k1 <= ni and ci >= k1 - k0
        assert (ci * q) % 8 == 0 and ci <= 65535
        assert ci * q * e * 2 <= limit
        if nxt is not None:
            assert nxt[0] == k1 and ci == k1 - k0
        else:
            assert ci - (k1 - k0) < 8
    # whole samples, every sample once, in order
    assert text_chunks[0][0] == 0 and text_chunks[-1][1] == nt
    cmax = max(ci for _, _, ci in image_chunks)
    for (m0, m1, r0, r1), nxt in zip(text_chunks, text_chunks[1:] + [None]):
        assert m0 < m1 <= nt and (r0, r1) == (cu[m0], cu[m1])
        if nxt is not None:
            assert nxt[0] == m1
        if m1 - m0 > 1:
            assert ops.maxsim_partial_bytes(cmax, q, r1 - r0) <= partial_bytes


def test_chunk_plan_expected_shapes():
    """the plans the issue's two gallery shapes get under the default limits"""
    ic, tc = ops.plan_maxsim_chunks(512, 196, 512, _cu(_counts(512, 77, 4)), 2 << 30)
    assert ic == [(0, 512, 512)] and len(tc) == 1
    ic, tc = ops.plan_maxsim_chunks(5000, 196, 512, _cu(_counts(25000, 77, 5)), 2 << 30)
    assert ic == [(0, 5000, 5000)] and len(tc) > 1 and min(r1 - r0 for _, _, r0, r1 in tc[:-1]) > 8192
    ic, tc = ops.plan_maxsim_chunks(5, 100, 256, _cu(_counts(7, 7, 1)), 2 << 30)
    assert ic == [(0, 5, 6)] and tc == [(0, 7, 0, sum(_counts(7, 7, 1)))]
    ic, _ = ops.plan_maxsim_chunks(5, 100, 256, _cu(_counts(7, 7, 1)), 12 * 4 * 16, 2 * 100 * 256 * 2)
    assert ic == [(0, 2, 2), (2, 4, 2), (4, 5, 2)]


def test_evaluate_as_original_clip_flag():
    assert parse_args(["--model", "ViT-B-16-colxlip"]).evaluate_as_original_clip is False
    assert parse_args(["--model", "ViT-B-16-colxlip", "--evaluate-as-original-clip"]).evaluate_as_original_clip is True


def test_score_fold_prototype_resolves():
    """the prototype added to include/clipx.h is parsed, exported by the library and bound with its argument types"""
    protos = {name: (res, args) for name, res, args in _lib.header_prototypes()}
    res, args = protos["clipx_maxsim_score_fold"]
    assert res is ctypes.c_int and len(args) == 16
    assert args[:5] == [ctypes.c_int] * 5 and args[5:9] == [ctypes.c_void_p] * 4
    assert args[9] is ctypes.c_long and args[11] is ctypes.c_long and args[12:15] == [ctypes.c_float] * 3
    assert hasattr(ctypes.CDLL(_lib.lib_path()), "clipx_maxsim_score_fold")
    fn = _lib.lib().clipx_maxsim_score_fold
    assert fn.restype is ctypes.c_int and list(fn.argtypes) == args


@pytest.mark.parametrize("q", [15, 16, 63, 64, 65535, 65536])
@pytest.mark.parametrize("e", [64, 96, 128, 192, 256, 320, 384, 512, 768])
def test_maxsim_gemm_takes_is_the_two_embed_dim_rules(q, e):
    """one rule on the bytes of an operand row (a multiple of the 128-byte k-step, at least two of them) against the rules the
    bf16 and the e4m3 route spelled out before, written out literally"""
    assert ops.maxsim_gemm_takes(q, e, 2) == (16 <= q <= 65535 and e % 64 == 0 and e >= 128)
    assert ops.maxsim_gemm_takes(q, e, 1) == (16 <= q <= 65535 and e % 128 == 0 and e >= 256)
