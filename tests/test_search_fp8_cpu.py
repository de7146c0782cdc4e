"""The e4m3 token index, the parts that need no GPU: a torch model of the row quantiser and its inverse, the chunk plan at one
byte per element, index storage and its files (contents put in through the model, the HIP quantiser needs a device), refusals,
the command line and the new C-ABI entry's prototype."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from colxlip_amd import _lib, ops
from colxlip_amd import search as S
from colxlip_amd.search import LateInteractionIndex
from tests.late_interaction_ref import counts_model, quant_model


def _rows(seed=0):
    """bf16 rows of many magnitudes, with the rule's corner cases: amax with fr = 0.875 exactly, just above, a power of two, an
    all-zero row, a row of one tiny value"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(40, 64, generator=g) * torch.logspace(-6, 4, 40).unsqueeze(1)
    x[0] = 0
    x[1] = 0
    x[1, 3] = 448.0             # fr = 0.875, ex = 9: e = 0, the byte is the largest finite e4m3
    x[2] = 0
    x[2, 5] = -0.875
    x[3] = 0
    x[3, 7] = 0.90625           # fr > 0.875: the next exponent
    x[4] = 0
    x[4, 0] = 1.0
    x[5] = 0
    x[5, 9] = 2.0 ** -100
    return x.to(torch.bfloat16)


def test_quantiser_model_and_its_inverse():
    x = _rows()
    b, e = quant_model(x)
    assert b.dtype == torch.uint8 and e.dtype == torch.int32 and b.shape == x.shape and e.shape == x.shape[:1]
    scaled = torch.ldexp(x.float(), -e.unsqueeze(-1))
    assert float(scaled.abs().max()) <= 448.0
    live = x.float().abs().amax(-1) > 0
    assert bool((scaled.abs().amax(-1)[live] > 224.0).all())                      # ... and e is the smallest such exponent
    assert int(e[1]) == 0 and int(b[1, 3]) == 0x7E and int(e[2]) == -9 and int(e[3]) == -8 and int(e[4]) == -8
    assert int(e[0]) == 0 and not bool(b[0].any())                                # all-zero row: zero bytes, exponent 0
    deq = ops.dequant_tokens_e4m3(b, e)
    assert deq.dtype == torch.float32 and deq.shape == x.shape
    # the inverse, independently: the byte's e4m3 value (sign, 4 exponent bits, bias 7, 3 mantissa bits) times 2^e in fp64
    bb = b.to(torch.int64)
    sign, ex, man = 1.0 - 2.0 * (bb >> 7).double(), (bb >> 3) & 15, (bb & 7).double()
    val = torch.where(ex == 0, man / 8 * 2.0 ** -6, (1 + man / 8) * torch.pow(2.0, (ex - 7).double())) * sign
    want = val * torch.pow(2.0, e.double()).unsqueeze(-1)
    assert torch.equal(deq.double(), want)
    assert torch.equal(deq.to(torch.bfloat16).float(), deq)                      # exact in bf16
    assert torch.equal(ops.dequant_tokens_e4m3(b, e, dtype=torch.bfloat16).float(), deq)
    # round to nearest: half an e4m3 step of the scaled value, 2^-4 relative or 2^-10 below the normal range
    err = (torch.ldexp(deq, -e.unsqueeze(-1)) - scaled).abs()
    assert bool((err <= torch.maximum(scaled.abs() * 2.0 ** -4, torch.tensor(2.0 ** -10))).all())
    # token form: [n, q, E] rows, one exponent per token
    t = x.view(5, 8, 64)
    tb, te = quant_model(t)
    assert te.shape == (5, 8) and torch.equal(ops.dequant_tokens_e4m3(tb, te).view(40, 64), deq)


@pytest.mark.parametrize("q", [16, 49, 196])
def test_chunk_plan_at_one_byte_per_element(q):
    e, ni = 256, 100000
    cu = list(range(0, 20 * 64 + 1, 20))                                          # 64 captions of 20 packed rows
    partial = 1 << 40                                                             # the partial arrays never decide here
    unit = 8 // int(np.gcd(q, 8))
    for limit in (None, 1 << 26, 1 << 24, 3 * q * e + 5):
        two, text2 = ops.plan_maxsim_chunks(ni, q, e, cu, partial, operand_bytes=limit, elem_bytes=2)
        one, text1 = ops.plan_maxsim_chunks(ni, q, e, cu, partial, operand_bytes=limit, elem_bytes=1)
        assert (two, text2) == ops.plan_maxsim_chunks(ni, q, e, cu, partial, operand_bytes=limit)       # the default is today's plan
        assert text1 == text2 == [(0, 64, 0, 1280)]
        cap = ops.MAXSIM_OPERAND_BYTES if limit is None else limit
        for plan, size in ((one, 1), (two, 2)):
            assert plan[0][0] == 0 and plan[-1][1] == ni and all(a[1] == b[0] for a, b in zip(plan, plan[1:]))
            for k0, k1, ci in plan:
                assert (ci * q) % 8 == 0 and ci <= ops.MAXSIM_MAX_IMAGES and k1 - k0 <= ci < k1 - k0 + unit
                assert ci * q * e * size <= cap or ci == unit                    # a limit below one unit of images still gets one unit
        c1, c2 = one[0][2], two[0][2]
        if limit in (1 << 26, 1 << 24):                                          # the operand limit decides: about twice the images
            assert c1 == cap // (q * e) // unit * unit and c2 == cap // (2 * q * e) // unit * unit
            assert 2 * c2 <= c1 <= 2 * c2 + unit
        assert c1 >= c2
    # the default limit at ViT-B/16-colxlip's 196 tokens x 512: 10 698 bf16 images per chunk, 21 398 e4m3 ones
    one, _ = ops.plan_maxsim_chunks(ni, 196, 512, cu, partial, elem_bytes=1)
    two, _ = ops.plan_maxsim_chunks(ni, 196, 512, cu, partial)
    assert one[0][2] == ops.MAXSIM_OPERAND_BYTES // (196 * 512) // 2 * 2 == 21398
    assert two[0][2] == ops.MAXSIM_OPERAND_BYTES // (2 * 196 * 512) // 2 * 2 == 10698


def _patch_quantiser(monkeypatch):
    calls = []
    monkeypatch.setattr(ops, "quant_tokens_e4m3", lambda t: (calls.append("quant"), quant_model(t))[1])
    monkeypatch.setattr(ops, "maxsim_text_counts", lambda t: (calls.append("counts"), counts_model(t))[1])
    return calls


def _captions(n, length, e, seed):
    g = torch.Generator().manual_seed(seed)
    t = torch.nn.functional.normalize(torch.randn(n, length, e, generator=g), dim=-1)
    for m in range(n):
        eot = 1 + (3 * m) % (length - 1)
        t[m, eot:] = t[m, eot]
    return t.to(torch.bfloat16)


@pytest.mark.parametrize("kind", ["image", "text"])
def test_fp8_index_add_save_load_round_trip(tmp_path, monkeypatch, kind):
    monkeypatch.setattr(LateInteractionIndex, "CHUNK_ITEMS", 8)
    monkeypatch.setattr(LateInteractionIndex, "IO_ITEMS", 5)
    calls = _patch_quantiser(monkeypatch)
    g = torch.Generator().manual_seed(1)
    feats = torch.randn(21, 32, generator=g)
    toks = _captions(21, 6, 32, 2)
    ids = torch.randperm(1000, generator=g)[:21].to(torch.int64)
    want_b, want_e = quant_model(toks)
    want_c = counts_model(toks)
    assert want_c.min() >= 2 and want_c.max() == 6 and len(set(want_c.tolist())) > 2
    index = LateInteractionIndex(kind, alpha=0.3, scale=17.5, device="cpu", token_dtype="fp8")
    for lo, hi in ((0, 3), (3, 16), (16, 21)):                                # adds that end inside, at and across chunk ends
        index.add(feats[lo:hi], toks[lo:hi] if lo else toks[lo:hi].float(), ids=ids[lo:hi])    # fp32 tokens: cast to bf16 first
    assert calls.count("quant") == 3 and calls.count("counts") == (3 if kind == "text" else 0)
    assert len(index) == 21 and index.has_tokens and [c[1].shape[0] for c in index.chunks()] == [8, 8, 5]

    def stored(ix):
        parts = list(zip(*[c[2] for c in ix.chunks()]))
        assert len(parts) == (3 if kind == "text" else 2)
        return [torch.cat(p) for p in parts]

    got = stored(index)
    assert got[0].dtype == torch.uint8 and torch.equal(got[0], want_b) and got[1].dtype == torch.int32 and torch.equal(got[1], want_e)
    assert kind == "image" or (got[2].dtype == torch.int32 and torch.equal(got[2], want_c))
    assert index.token_bytes() == 21 * (6 * 32 + 6 * 4 + (4 if kind == "text" else 0))       # bytes + exponents (+ counts) as allocated
    path = index.save(str(tmp_path / "idx"))
    files = sorted(S._FILES + S._FP8_FILES[:2 if kind == "text" else 1])
    assert sorted(os.listdir(path)) == files
    with open(os.path.join(path, "meta.json")) as f:
        meta = json.load(f)
    assert meta["kind"] == kind and meta["alpha"] == 0.3 and meta["scale"] == 17.5 and meta["n"] == 21
    assert meta["tokens"] == [6, 32] and meta["token_dtype"] == "e4m3"
    on_disk = np.load(os.path.join(path, "tokens.npy"))
    assert on_disk.dtype == np.uint8 and on_disk.shape == (21, 6, 32) and np.array_equal(on_disk, want_b.numpy())
    exps = np.load(os.path.join(path, "token_exp.npy"))
    assert exps.dtype == np.int32 and np.array_equal(exps, want_e.numpy())
    if kind == "text":
        assert np.array_equal(np.load(os.path.join(path, "token_cnt.npy")), want_c.numpy())
    n_calls = len(calls)
    back = LateInteractionIndex.load(path, device="cpu")
    assert len(calls) == n_calls                                                 # kept as saved: nothing is quantised again
    assert (back.kind, back.alpha, back.scale, len(back), back.token_dtype) == (kind, 0.3, 17.5, 21, "fp8")
    assert torch.equal(back.ids, ids) and not back._running_ids
    assert torch.equal(torch.cat([c[1] for c in back.chunks()]), feats)
    assert all(torch.equal(a, b) and a.dtype == b.dtype for a, b in zip(stored(back), got))
    # saving over it as a default index removes the fp8 files
    plain = LateInteractionIndex(kind, alpha=0.3, scale=17.5, device="cpu")
    plain.add(feats, toks)
    plain.save(path)
    assert sorted(os.listdir(path)) == sorted(S._FILES)
    again = LateInteractionIndex.load(path, device="cpu")
    assert again.token_dtype is None and again._running_ids and again.chunks()[0][2].dtype == torch.bfloat16
    assert torch.equal(torch.cat([c[2] for c in again.chunks()]).view(torch.int16), toks.view(torch.int16))


def test_fp8_index_running_ids_and_default_directory(tmp_path, monkeypatch):
    _patch_quantiser(monkeypatch)
    feats, toks = torch.randn(5, 16), _captions(5, 4, 16, 3)
    index = LateInteractionIndex("image", alpha=0.5, device="cpu", token_dtype="fp8").add(feats[:2], toks[:2]).add(feats[2:], toks[2:])
    assert index._running_ids and index.ids.tolist() == [0, 1, 2, 3, 4]
    back = LateInteractionIndex.load(index.save(str(tmp_path / "a")), device="cpu")
    assert back._running_ids and back.token_dtype == "fp8" and torch.equal(back.chunks()[0][2][0], quant_model(toks)[0])
    default = LateInteractionIndex("image", alpha=0.5, device="cpu").add(feats, toks)
    assert default.token_dtype is None and default.chunks()[0][2].dtype == torch.bfloat16
    path = default.save(str(tmp_path / "b"))
    with open(os.path.join(path, "meta.json")) as f:
        assert json.load(f)["token_dtype"] == "bfloat16"
    assert LateInteractionIndex.load(path, device="cpu").token_dtype is None
    # alpha = 1 never reads tokens: nothing is quantised or stored
    glob = LateInteractionIndex("image", alpha=1.0, device="cpu", token_dtype="fp8").add(feats, toks)
    assert not glob.has_tokens and glob.token_bytes() == 0


def test_fp8_refusals(monkeypatch):
    _patch_quantiser(monkeypatch)
    with pytest.raises(ValueError, match="token_dtype"):
        LateInteractionIndex(token_dtype="int8", device="cpu")
    with pytest.raises(ValueError, match="token_dtype"):
        LateInteractionIndex("text", token_dtype="e4m3", device="cpu")
    feats, toks = torch.randn(4, 16), _captions(4, 6, 16, 5)
    index = LateInteractionIndex("text", alpha=0.5, device="cpu", token_dtype="fp8").add(feats, toks)
    with pytest.raises(ValueError, match="dtype"):
        index.add(feats, toks.to(torch.float16))
    with pytest.raises(ValueError, match="shape or dtype"):
        index.add(feats, toks[:, :5])
    with pytest.raises(ValueError, match="tokens must be"):
        index.add(feats, toks[:3])
    with pytest.raises(ValueError, match="stored form"):
        index.add(feats, quant_model(toks))                                     # a text gallery's stored form has cnt too
    with pytest.raises(ValueError, match="stored form"):
        index.add(feats, (toks, quant_model(toks)[1], counts_model(toks)))
    assert len(index) == 4
    index.add(feats, quant_model(toks) + (counts_model(toks),))                  # the stored form itself is taken as it is
    assert len(index) == 8 and torch.equal(index.chunks()[0][2][0][4:], index.chunks()[0][2][0][:4])
    with pytest.raises(ValueError, match="alpha"):
        LateInteractionIndex("image", alpha=0.5, device="cpu", token_dtype="fp8").add(feats)


def test_cli_index_dtype():
    base = ["--model", "ViT-B-32-colxlip", "--dataset-type", "synthetic", "--retrieval-coco"]
    assert S.parse_args(base).index_dtype == "model"
    assert S.parse_args(base + ["--index-dtype", "fp8", "--save-index", "d"]).index_dtype == "fp8"
    assert S.parse_args(base + ["--index-dtype", "model"]).index_dtype == "model"
    with pytest.raises(SystemExit):
        S.parse_args(base + ["--index-dtype", "int8"])


def test_fp8_entry_prototype_and_refusals():
    protos = {name: (res, args) for name, res, args in _lib.header_prototypes()}
    res, args = protos["clipx_maxsim_gemm_fp8"]
    assert res is ctypes.c_int and args == [ctypes.c_int] * 4 + [ctypes.c_void_p] * 6 + [ctypes.c_int, ctypes.c_void_p]
    assert hasattr(ctypes.CDLL(_lib.lib_path()), "clipx_maxsim_gemm_fp8")
    fn = _lib.lib().clipx_maxsim_gemm_fp8
    # shapes the kernel does not take are errors, reported before anything is launched: nothing falls back inside the library
    for R, ni, q, e, ld in ((4, 2, 16, 64, 16), (4, 2, 16, 320, 16), (4, 2, 16, 128, 16), (4, 2, 8, 256, 16), (40, 2, 16, 256, 16)):
        assert fn(R, ni, q, e, None, None, None, None, None, None, ld, None) != 0
        assert b"maxsim_gemm_fp8" in _lib.lib().clipx_last_error()
    assert fn(4, 2, 16, 256, None, None, None, None, None, None, 16, None) != 0 and b"null" in _lib.lib().clipx_last_error()
    assert fn(0, 2, 16, 256, None, None, None, None, None, None, 16, None) == 0
    # the Python side says which route runs, and refuses CPU tensors on the kernel's wrappers
    b8, e8 = quant_model(_captions(2, 16, 256, 1))
    assert not ops.maxsim_fp8_applies((b8, e8), (b8, e8, counts_model(_captions(2, 16, 256, 1))))       # CPU tensors
    with pytest.raises(RuntimeError, match="no CPU"):
        ops.quant_tokens_e4m3(_captions(2, 16, 256, 1))
