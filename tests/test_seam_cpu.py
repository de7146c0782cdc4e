"""The Python seam: what the reference's entry point imports and reads must exist here under the same names.

Half of these tests check against `tests/golden/seam.json`: names read with `ast` from the reference's `src/main.py` and
`colxlip/{__init__,factory,loss,train,data,params,model}.py` (`make_golden.py seam`; nothing of it is executed and no source
text is stored).  They prove exactly this, and INTEGRATION.md claims no more: with this repository on sys.path, every
`from colxlip... import ...` of the reference's `main.py` resolves, every `args.<flag>` it reads is produced by
`colxlip.params.parse_args`, by `init_distributed_device`, or by `main.py` itself, and the functions it calls take the
arguments it passes.  `main.py`'s other imports (`open_clip_train.*`, `huggingface_hub`, `wandb`) are third-party packages of
the reference's environment."""
import ast
import inspect
import json
import os

import numpy as np
import pytest
import torch

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "seam.json")) as _f:
    SEAM = json.load(_f)


# ------------------------------------------------------------------ imports of the reference's main.py
def test_every_colxlip_import_of_reference_main_resolves():
    import importlib
    seen = 0
    for node in SEAM["main_colxlip_imports"]:
        mod = importlib.import_module(node["module"])
        for name in node["names"]:
            assert hasattr(mod, name), f"{node['module']}.{name} (main.py:{node['line']}) does not exist here"
            seen += 1
    assert seen >= 7          # parse_args, create_model_and_transforms, get_tokenizer, create_loss, train_one_epoch, evaluate, get_data


def test_colxlip_is_an_alias_not_a_copy():
    import colxlip
    import colxlip_amd
    for name in colxlip.ALIASED:
        assert getattr(colxlip, name) is getattr(colxlip_amd, name)
    with pytest.raises(ModuleNotFoundError):
        import colxlip.transformer  # noqa: F401  (no counterpart: absent on purpose)


def test_reference_package_root_exports_exist():
    """Every name `src/colxlip/__init__.py` re-exports is importable from `colxlip` (a name whose subsystem is not built
    raises when CALLED, with a message; it is not silently missing)."""
    import colxlip
    for name in SEAM["root_exports"]:
        assert hasattr(colxlip, name), name
    with pytest.raises(NotImplementedError):
        colxlip.trace_model(None)
    with pytest.raises(RuntimeError):
        colxlip.download_weights_from_hf("repo", "file")


# ------------------------------------------------------------------ flags
def _provided_by_init_distributed_device():
    """What this stack's init_distributed_device sets on args (the reference's is open_clip_train's)."""
    import argparse
    from colxlip.distributed import init_distributed_device
    ns = argparse.Namespace(device="cpu", dist_backend="gloo", dist_url="env://", no_set_device_rank=False)
    before = set(vars(ns))
    init_distributed_device(ns)
    return set(vars(ns)) - before | {"device"}


def test_every_flag_reference_main_reads_is_defined():
    from colxlip.params import parse_args
    reads = set(SEAM["main_args_read"])
    own = set(SEAM["main_args_set"])                     # args.name / log_path / wandb / checkpoint_path / save_logs / ...
    parsed = set(vars(parse_args([])))
    dist = _provided_by_init_distributed_device()
    assert {"distributed", "rank", "local_rank", "world_size", "device"} <= dist
    missing = sorted(reads - parsed - own - dist)
    assert not missing, f"reference main.py reads args.{missing} which parse_args does not define"
    # and the defaults of the flags whose subsystems are not built here are the reference's inert ones
    d = parse_args([])
    assert d.remote_sync is None and d.copy_codebase is False and d.huggingface_model_name == "" and d.use_bnb_linear is None
    assert d.report_to == "" and d.val_data is None and d.debug is False and d.log_local is False
    assert d.remote_sync_frequency == 300 and d.remote_sync_protocol == "s3" and d.wandb_project_name == "open-clip"


def test_flags_read_by_reference_train_loop_and_evaluate_are_defined():
    from colxlip.params import parse_args
    parsed = set(vars(parse_args([]))) | _provided_by_init_distributed_device() | set(SEAM["main_args_set"])
    for fn_name in ("train_one_epoch", "evaluate", "retrieval_on_split"):
        missing = sorted(set(SEAM["train_args_read"][fn_name]) - parsed)
        assert not missing, (fn_name, missing)


def test_unsupported_flag_values_are_reported_not_ignored():
    from colxlip_amd.params import parse_args, unsupported_flag_values
    assert unsupported_flag_values(parse_args(["--model", "ViT-B-32"])) == []
    bad = dict(unsupported_flag_values(parse_args(["--remote-sync", "s3://x", "--copy-codebase", "--report-to", "wandb",
                                                    "--huggingface-model-name", "m.pt"])))
    assert set(bad) == {"remote_sync", "copy_codebase", "report_to", "huggingface_model_name"}
    assert unsupported_flag_values(parse_args(["--report-to", "tensorboard"])) == []


def test_model_family_adam_defaults():
    from colxlip_amd.params import parse_args
    a = parse_args(["--model", "ViT-B-32"])
    assert (a.lr, a.beta1, a.beta2, a.eps) == (5.0e-4, 0.9, 0.98, 1.0e-6)
    a = parse_args(["--model", "RN50", "--lr", "1e-3"])
    assert (a.lr, a.beta1, a.beta2, a.eps) == (1e-3, 0.9, 0.999, 1.0e-8)
    assert parse_args(["--aug-cfg", "scale=(0.4,1.0)", "color_jitter=0.3", "mode=x"]).aug_cfg == {
        "scale": (0.4, 1.0), "color_jitter": 0.3, "mode": "x"}


# ------------------------------------------------------------------ call signatures
@pytest.mark.parametrize("rel,cls,fn,ours", [
    ("colxlip/factory.py", None, "create_model", "colxlip.factory:create_model"),
    ("colxlip/factory.py", None, "create_model_and_transforms", "colxlip.factory:create_model_and_transforms"),
    ("colxlip/factory.py", None, "create_loss", "colxlip.factory:create_loss"),
    ("colxlip/factory.py", None, "get_tokenizer", "colxlip.factory:get_tokenizer"),
    ("colxlip/factory.py", None, "load_checkpoint", "colxlip.factory:load_checkpoint"),
    ("colxlip/factory.py", None, "load_state_dict", "colxlip.factory:load_state_dict"),
    ("colxlip/loss.py", None, "gather_features", "colxlip.loss:gather_features"),
    ("colxlip/loss.py", None, "compute_colbert_similarity", "colxlip.loss:compute_colbert_similarity"),
    ("colxlip/loss.py", "ClipLoss", "__init__", "colxlip.loss:ClipLoss.__init__"),
    ("colxlip/loss.py", "ClipLoss", "get_ground_truth", "colxlip.loss:ClipLoss.get_ground_truth"),
    ("colxlip/loss.py", "ClipLoss", "get_logits", "colxlip.loss:ClipLoss.get_logits"),
    ("colxlip/loss.py", "ClipLoss", "forward", "colxlip.loss:ClipLoss.forward"),
    ("colxlip/loss.py", "ColClipLoss", "__init__", "colxlip.loss:ColClipLoss.__init__"),
    ("colxlip/train.py", None, "train_one_epoch", "colxlip.train:train_one_epoch"),
    ("colxlip/train.py", None, "evaluate", "colxlip.train:evaluate"),
    ("colxlip/train.py", None, "compute_retrieval", "colxlip.train:compute_retrieval"),
    ("colxlip/train.py", None, "retrieval_on_split", "colxlip.train:retrieval_on_split"),
    ("colxlip/data.py", None, "get_data", "colxlip.data:get_data"),
    ("colxlip/params.py", None, "parse_args", "colxlip.params:parse_args"),
    ("colxlip/model.py", None, "convert_weights_to_lp", "colxlip.model:convert_weights_to_lp"),
    ("colxlip/model.py", None, "get_cast_dtype", "colxlip.model:get_cast_dtype"),
    ("colxlip/model.py", None, "get_input_dtype", "colxlip.model:get_input_dtype"),
])
def test_signatures_accept_what_the_reference_passes(rel, cls, fn, ours):
    """Parameter names, in order, of the reference's definition are a prefix of ours (ours may add trailing keyword
    arguments with defaults: `grad_sync=` on train_one_epoch, `model=` on get_data), and the defaults agree."""
    import importlib
    ref = SEAM["signatures"][f"{rel}:{cls + '.' if cls else ''}{fn}"]
    mod_name, _, path = ours.partition(":")
    obj = importlib.import_module(mod_name)
    for part in path.split("."):
        obj = getattr(obj, part)
    sig = inspect.signature(obj)
    mine = [p.name for p in sig.parameters.values() if p.kind not in (p.VAR_KEYWORD, p.VAR_POSITIONAL)]
    want = ref["params"]
    assert mine[:len(want)] == want, (ours, want, mine)
    for extra in mine[len(want):]:
        assert sig.parameters[extra].default is not inspect.Parameter.empty, (ours, extra)
    assert ref["var_keyword"] == any(p.kind == p.VAR_KEYWORD for p in sig.parameters.values()), ours
    # defaults: compare the literal ones (the fixture keeps only those; torch.float16 etc. are left out)
    for name, text in ref["literal_defaults"].items():
        val = ast.literal_eval(text)
        assert sig.parameters[name].default == val, (ours, name, val, sig.parameters[name].default)


# ------------------------------------------------------------------ a2: convert_weights_to_lp against the reference's run
def test_convert_weights_to_lp_matches_reference_fixture(golden_dir):
    """tests/golden/lp_convert.npz = the reference's own convert_weights_to_lp on the reference's towers (make_golden.golden_lp).
    Same set of cast tensors; same values afterwards, tensor for tensor, bit for bit."""
    from colxlip_amd import create_model, convert_weights_to_lp
    from colxlip_amd.model import lp_parameter_names
    from oracle import clip_oracle as O
    z = np.load(os.path.join(golden_dir, "lp_convert.npz"), allow_pickle=False)
    model = create_model("ViT-tiny-test", precision="fp32", device="cpu")
    sd = O.perturb_state_dict(O.init_state_dict(O.TINY, seed=0), seed=1)
    model.load_state_dict(sd)
    assert sorted(lp_parameter_names(model)) == [str(n) for n in z["cast_names"]]
    convert_weights_to_lp(model, dtype=torch.bfloat16)
    assert model.compute_dtype == torch.bfloat16                 # a parity-mode model is switched to bf16 operands
    after = model.state_dict()
    for name in z["all_names"]:
        name = str(name)
        assert after[name].dtype == torch.float32                # storage stays fp32 (masters)
        assert torch.equal(after[name], torch.from_numpy(z["after/" + name])), name
    with pytest.raises(NotImplementedError):
        convert_weights_to_lp(model, dtype=torch.float16)


# ------------------------------------------------------------------ host-side pieces of the eval path
def test_hash_tokenizer_contract():
    from colxlip_amd.factory import HashTokenizer
    tok = HashTokenizer(context_length=16, vocab_size=1000)
    ids = tok(["a photo of a cat", "word " * 40, ""])
    assert ids.shape == (3, 16) and ids.dtype == torch.long
    assert ids[0, 0] == 998 and ids[0, 6] == 999 and int(ids[0, 7:].sum()) == 0
    assert ids[1, -1] == 999 and ids[1].argmax() == 15          # truncated rows still pool at the last position
    assert ids[2, :2].tolist() == [998, 999]
    assert torch.equal(tok("a photo of a cat"), ids[:1]) and int(ids.max()) == 999
    assert tok(["x"], context_length=8).shape == (1, 8)


def test_synthetic_retrieval_split_and_remap():
    from colxlip_amd.data import synthetic_retrieval_split
    from colxlip_amd.train import remap_indices
    txt, img, img2txt, txt2img = synthetic_retrieval_split(6, 5, 32, context_length=20, vocab_size=512, batch_size=4)
    assert txt.dataloader.num_samples == 30 and img.dataloader.num_samples == 6
    assert txt.dataloader.num_batches == 8 and img.dataloader.num_batches == 2
    ids = torch.cat([i for _, i in img.dataloader])
    caps = torch.cat([c for _, c in txt.dataloader])
    assert sorted(ids.tolist()) != ids.tolist()                    # arbitrary ids in shuffled order
    for texts, _ in txt.dataloader:
        assert texts.ndim == 2 and texts.shape[1] == 20 and int((texts == 511).sum(1).min()) == 1
    i2t, t2i = remap_indices(ids, caps, img2txt, txt2img)
    assert sorted(i2t) == list(range(6)) and all(i2t[r] == list(range(5 * r, 5 * r + 5)) for r in range(6))
    assert [t2i[c] for c in range(30)] == [c // 5 for c in range(30)]
    with pytest.raises(ValueError):
        remap_indices(ids, caps.flip(0), img2txt, txt2img)


def test_get_data_takes_the_reference_call_form():
    """`get_data(args, (preprocess_train, preprocess_val), epoch=..., tokenizer=...)` (reference main.py:326-331): the image
    size comes from the transforms the factory returned."""
    from colxlip_amd import create_model_and_transforms, get_tokenizer
    from colxlip_amd.data import get_data
    from colxlip_amd.params import parse_args
    args = parse_args(["--model", "ViT-tiny-test", "--dataset-type", "synthetic", "--batch-size", "4", "--train-num-samples", "16",
                       "--retrieval-coco", "--val-num-samples", "8", "--device", "cpu"])
    args.rank, args.world_size = 0, 1
    model, pre_t, pre_v = create_model_and_transforms(args.model, precision="fp32", device="cpu")
    data = get_data(args, (pre_t, pre_v), epoch=0, tokenizer=get_tokenizer(args.model))
    assert set(data) == {"train", "retrieval_coco"}
    images, texts = next(iter(data["train"].dataloader))
    assert images.shape[-2:] == tuple(model.visual.image_size) and texts.shape[1:] == (1, 77)
    txt, img, i2t, t2i = data["retrieval_coco"]
    assert img.dataloader.num_samples == 8 and txt.dataloader.num_samples == 40
    args2 = parse_args(["--dataset-type", "csv"])
    args2.rank, args2.world_size = 0, 1
    with pytest.raises(ValueError):
        get_data(args2, (pre_t, pre_v))
