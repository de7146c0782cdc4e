"""Command-line flags of the train / eval entry point, with the reference's names and defaults
(reference params.py:33-986; Adam defaults by model family params.py:12-18,982-986).

The flags are a TABLE (`_FLAGS`): name -> argparse keywords.  Three groups:
  * flags the hot path acts on (model, precision, batch, optimiser, schedule, loss mode, checkpoints, logging);
  * flags the reference's `main.py` / `train.py` READ but whose subsystems are outside this stack (wandb, remote sync, HF
    download, int8 linear, FLAIR inference, zero-shot sets): they parse, keep the reference's inert default, and
    `unsupported_flag_values()` names the ones a caller set to something this stack cannot honour;
  * two flags of this stack's own (`--ddp-wrap`, `--grad-comm-dtype`).
`tests/test_seam_cpu.py` reads the reference's `main.py` and asserts that every `args.<flag>` it touches exists here."""
import argparse
import ast

_DATASET_TYPES = ["webdataset", "csv", "synthetic", "auto", "coco", "flickr", "packed"]
_PRECISIONS = ["amp", "amp_bf16", "amp_bfloat16", "bf16", "fp16", "pure_bf16", "pure_fp16", "fp32", "fp8", "fp8_mfma"]


def get_default_params(model_name):
    """Adam hyper-parameters of the CLIP paper by model family (reference params.py:12-18)."""
    vit = "vit" in model_name.lower()
    return {"lr": 5.0e-4, "beta1": 0.9, "beta2": 0.98 if vit else 0.999, "eps": 1.0e-6 if vit else 1.0e-8}


class ParseKwargs(argparse.Action):
    """`--aug-cfg key=value ...` -> dict, values parsed as Python literals where they are ones."""

    def __call__(self, parser, namespace, values, option_string=None):
        parsed = {}
        for item in values:
            key, _, raw = item.partition('=')
            try:
                parsed[key] = ast.literal_eval(raw)
            except (ValueError, SyntaxError):
                parsed[key] = raw
        setattr(namespace, self.dest, parsed)


def _flag(default=False):
    return {"action": "store_true", "default": default}


_FLAGS = {
    # ---- data
    "--train-data": dict(type=str, default=None),
    "--val-data": dict(type=str, default=None),
    "--train-num-samples": dict(type=int, default=None),
    "--val-num-samples": dict(type=int, default=None),
    "--dataset-type": dict(choices=_DATASET_TYPES, default="coco"),
    "--dataset-resampled": _flag(),
    "--workers": dict(type=int, default=4),
    "--batch-size": dict(type=int, default=64),
    "--retrieval-coco": _flag(),          # with --dataset-type synthetic: a synthetic retrieval split under the same key
    "--retrieval-flickr": _flag(),
    "--imagenet-val": dict(type=str, default=None),
    "--imagenet-v2": dict(type=str, default=None),
    # ---- experiment / logging
    "--logs-dir": dict(type=str, default="./logs/"),
    "--log-local": _flag(),
    "--name": dict(type=str, default=None),
    "--report-to": dict(type=str, default=''),
    "--wandb-notes": dict(type=str, default=''),
    "--wandb-project-name": dict(type=str, default='open-clip'),
    "--debug": _flag(),
    "--copy-codebase": _flag(),
    "--log-every-n-steps": dict(type=int, default=100),
    "--remote-sync": dict(type=str, default=None),
    "--remote-sync-frequency": dict(type=int, default=300),
    "--remote-sync-protocol": dict(choices=["s3", "fsspec"], default="s3"),
    # ---- schedule / optimiser
    "--epochs": dict(type=int, default=32),
    "--epochs-cooldown": dict(type=int, default=None),
    "--lr": dict(type=float, default=None),
    "--beta1": dict(type=float, default=None),
    "--beta2": dict(type=float, default=None),
    "--eps": dict(type=float, default=None),
    "--wd": dict(type=float, default=0.2),
    "--warmup": dict(type=int, default=10000),
    "--skip-scheduler": _flag(),
    "--lr-scheduler": dict(type=str, default='cosine'),
    "--lr-cooldown-end": dict(type=float, default=0.0),
    "--lr-cooldown-power": dict(type=float, default=1.0),
    "--accum-freq": dict(type=int, default=1),
    "--grad-clip-norm": dict(type=float, default=None),
    "--seed": dict(type=int, default=0),
    # ---- checkpoints / evaluation cadence
    "--save-frequency": dict(type=int, default=1),
    "--save-most-recent": _flag(),
    "--delete-previous-checkpoint": _flag(),
    "--zeroshot-frequency": dict(type=int, default=2),
    "--val-frequency": dict(type=int, default=1),
    "--resume": dict(type=str, default=None),
    # ---- model
    "--precision": dict(choices=_PRECISIONS, default="amp"),
    "--model": dict(type=str, default="RN50"),
    "--pretrained": dict(type=str, default=''),
    "--pretrained-image": _flag(),
    "--huggingface-model-name": dict(type=str, default=""),
    "--huggingface-repo-name": dict(type=str, default=""),
    "--image-mean": dict(type=float, nargs='+', default=None, metavar='MEAN'),
    "--image-std": dict(type=float, nargs='+', default=None, metavar='STD'),
    "--image-interpolation": dict(type=str, default=None, choices=['bicubic', 'bilinear', 'random']),
    "--image-resize-mode": dict(type=str, default=None, choices=['shortest', 'longest', 'squash']),
    "--aug-cfg": dict(nargs='*', default={}, action=ParseKwargs),
    "--grad-checkpointing": _flag(),
    "--force-image-size": dict(type=int, nargs='+', default=None),
    "--force-quick-gelu": _flag(),
    "--force-patch-dropout": dict(type=float, default=None),
    "--force-custom-text": _flag(),
    "--torchscript": _flag(),
    "--torchcompile": _flag(),
    # extension (not a reference flag): ColClipLoss computes only this rank's text rows of the token logits (loss.ColClipLoss)
    "--colclip-rows-local": _flag(),
    "--trace": _flag(),
    "--use-bn-sync": _flag(),
    "--use-bnb-linear": dict(default=None),
    "--lock-image": _flag(),
    "--lock-text": _flag(),
    "--distill-model": dict(default=None),
    "--distill-pretrained": dict(default=None),
    "--inference-with-flair": _flag(),
    # a ColXLIP model is scored on its global features only (the reference's `original_clip` mode; the same as --alpha 1)
    "--evaluate-as-original-clip": _flag(),
    # ---- loss
    "--local-loss": _flag(),
    "--gather-with-grad": _flag(),
    "--alpha": dict(type=float, default=0.5),
    "--siglip": _flag(),
    "--loss-dist-impl": dict(type=str, default=None, choices=["bidir", "shift", "reduce", "gather"],
                             help="SigLipLoss's exchange of the text features between ranks (open_clip's flag; default bidir)"),
    # ---- distributed
    "--dist-url": dict(type=str, default="env://"),
    "--dist-backend": dict(type=str, default="nccl"),
    "--horovod": _flag(),
    "--ddp-static-graph": _flag(),
    "--no-set-device-rank": _flag(),
    "--device": dict(type=str, default="cuda"),
    # ---- this stack's own
    "--ddp-wrap": dict(action="store_true", default=False,
                       help="wrap the model in DistributedDataParallel exactly as the reference's main.py does"),
    "--grad-comm-dtype": dict(default="fp32", choices=["fp32", "bf16"],
                              help="wire format of the parameter-gradient all-reduce (accumulation stays fp32)"),
    "--shard-optimizer": dict(action="store_true", default=False,
                              help="ZeRO-1: reduce-scatter the gradient arenas, AdamW on each rank's slices, all-gather the parameters"),
}

# value a flag must keep for this stack to honour it: the subsystem behind any other value is not built here
_INERT_ONLY = {
    "remote_sync": None, "copy_codebase": False, "huggingface_model_name": "", "use_bnb_linear": None,
    "horovod": False, "torchscript": False, "trace": False, "lock_image": False, "lock_text": False,
    "inference_with_flair": False,
    "imagenet_val": None, "imagenet_v2": None, "use_bn_sync": False, "dataset_resampled": False,
    "torchcompile": False,        # no tracing compiler in this stack (hand-written kernels behind autograd Functions)
}


def unsupported_flag_values(args):
    """[(flag, value)] of the flags that were moved off their inert default although this stack has no such subsystem
    (`main` refuses to start with any), plus `wandb` in --report-to."""
    bad = [(name, getattr(args, name)) for name, inert in _INERT_ONLY.items() if getattr(args, name, inert) != inert]
    if any(tok in ("wandb", "all") for tok in str(getattr(args, "report_to", "")).split(",")):
        bad.append(("report_to", args.report_to))
    return bad


def build_parser():
    parser = argparse.ArgumentParser()
    for name, kw in _FLAGS.items():
        parser.add_argument(name, **kw)
    return parser


def parse_args(args):
    args = build_parser().parse_args(args)
    for name, val in get_default_params(args.model).items():      # model-family Adam defaults where none was passed
        if getattr(args, name) is None:
            setattr(args, name, val)
    return args
