"""Train / eval entry point for the plain-CLIP hot path; the flag set, experiment layout (logs-dir/name/{out.log, params.txt,
checkpoints/epoch_K.pt, checkpoints/results.jsonl}), checkpoint dict keys and resume rules are the reference's
(src/main.py:79-441), the structure is this stack's: one `_Run` object whose methods are the stages.

    python -m colxlip_amd.main --model ViT-B-32 --dataset-type synthetic --batch-size 512 \
        --precision amp_bf16 --epochs 1 --train-num-samples 51200 --local-loss --gather-with-grad [--retrieval-coco]

Differences from the reference's runner, all deliberate: gradient averaging is `distributed.GradSync` on the towers' flat
arenas (`--ddp-wrap` restores the literal DistributedDataParallel wrap), the optimizer is the one-launch `FusedAdamW`
(same grouping and state-dict keys), there is no GradScaler (bf16 needs none), and flags whose subsystems are not built
here (`params.unsupported_flag_values`) stop the run with a message instead of being ignored."""
import glob
import logging
import math
import os
import random
import re
import sys
from datetime import datetime

import numpy as np
import torch

from .data import get_data
from .distributed import GradSync, broadcast_object, init_distributed_device, is_master
from .factory import create_loss, create_model, create_model_and_transforms, distill_enabled, get_model_config
from .optim import FusedAdamW, ShardedAdamW, param_groups
from .params import parse_args, unsupported_flag_values
from . import scheduler as schedules
from .train import RETRIEVAL_SPLITS, evaluate, train_one_epoch

LATEST_CHECKPOINT_NAME = "epoch_latest.pt"


def random_seed(seed=42, rank=0):
    torch.manual_seed(seed + rank)
    np.random.seed(seed + rank)
    random.seed(seed + rank)


def _checkpoint_order(path: str):
    return [int(tok) if tok.isdigit() else tok for tok in re.split(r"(\d+)", path.lower())]


def get_latest_checkpoint(path: str):
    """Newest `*.pt` below `path` in natural order (epoch_9 < epoch_10), or None (reference main.py:54-67, local branch;
    remote/S3 listing is outside this stack)."""
    found = glob.glob(os.path.join(path, "**", "*.pt"), recursive=True)
    found = [f for f in found if os.path.basename(f) != "tmp.pt"]
    return max(found, key=_checkpoint_order) if found else None


def distill_refusal(args):
    """Why `main` cannot distil with these flags, or None.  EXTENSION: the reference parses --distill-model /
    --distill-pretrained but its main.py:214 hard-wires `dist_model = None`; here they build a teacher the way open_clip's
    trainer does.  Every check reads only the flags and the model configs (no device)."""
    model, pretrained = getattr(args, "distill_model", None), getattr(args, "distill_pretrained", None)
    if not model and not pretrained:
        return None
    if not (model and pretrained):
        return "distillation needs both --distill-model and --distill-pretrained"
    if int(getattr(args, "accum_freq", 1)) > 1:
        return "distillation does not support --accum-freq > 1"
    if getattr(args, "siglip", False):
        return "distillation does not support --siglip"
    for role, name in (("student", args.model), ("teacher", model)):
        if "colxlip" in name.lower():
            return f"distillation needs CLIP models: the {role} {name} is a ColXLIP model"
        if "coca" in name.lower():
            return f"distillation does not support CoCa models (the {role} is {name})"
    s_cfg, t_cfg = get_model_config(args.model.replace("/", "-")), get_model_config(model.replace("/", "-"))
    if t_cfg is None:
        return f"teacher model {model} not found"
    if s_cfg is None:
        return None                 # create_model reports an unknown student itself

    def size(cfg, forced=None):
        v = forced or cfg["vision_cfg"]["image_size"]
        v = v[0] if isinstance(v, (list, tuple)) and len(v) == 1 else v
        return tuple(v) if isinstance(v, (list, tuple)) else (v, v)

    forced = getattr(args, "force_image_size", None)
    for what, sv, tv in (("image size", size(s_cfg, forced), size(t_cfg)),
                         ("context length", s_cfg["text_cfg"].get("context_length", 77), t_cfg["text_cfg"].get("context_length", 77)),
                         ("vocabulary size", s_cfg["text_cfg"].get("vocab_size", 49408), t_cfg["text_cfg"].get("vocab_size", 49408))):
        if sv != tv:
            return f"the teacher sees the student's batch: its {what} {tv} differs from the student's {sv}"
    return None


class _Run:
    def __init__(self, argv):
        self.args = parse_args(argv)
        self.device = init_distributed_device(self.args)
        self.master = is_master(self.args)
        self.model = self.core = self.grad_sync = self.optimizer = self.scheduler = None
        self.dist_model = None
        self.data, self.start_epoch, self.writer = {}, 0, None

    # ---- experiment directory, logging, resume target ------------------------------------------------------------
    def open_experiment(self) -> bool:
        a = self.args
        logging.basicConfig(format="%(asctime)s | %(levelname)s | %(message)s")   # no-op when the host app configured logging
        logging.getLogger().setLevel((logging.DEBUG if a.debug else logging.INFO) if self.master else logging.WARN)
        bad = unsupported_flag_values(a)
        if bad:
            logging.error("flags outside this stack: " + ", ".join(f"--{k.replace('_', '-')}={v!r}" for k, v in bad))
            return False
        why = distill_refusal(a)
        if why:
            logging.error(why)
            return False
        if a.name is None:
            stamp = broadcast_object(a, datetime.now().strftime("%Y_%m_%d-%H_%M_%S"))
            a.name = '-'.join([stamp, f"model_{a.model.replace('/', '-')}", f"lr_{a.lr}", f"b_{a.batch_size}",
                               f"j_{a.workers}", f"p_{a.precision}"])
        base = os.path.join(a.logs_dir, a.name)
        a.checkpoint_path = os.path.join(base, "checkpoints")
        a.save_logs = bool(a.logs_dir) and a.logs_dir.lower() != 'none' and self.master
        a.wandb = False
        a.tensorboard = any(tok in ("tensorboard", "all") for tok in a.report_to.split(","))
        a.tensorboard_path = os.path.join(base, "tensorboard") if (a.tensorboard and self.master) else ''
        a.log_path = None
        if is_master(a, local=a.log_local):
            os.makedirs(base, exist_ok=True)
            a.log_path = os.path.join(base, f'out-{a.rank}' if a.log_local else 'out.log')
            if os.path.exists(a.log_path) and a.resume != 'latest':
                print(f"Error. Experiment already exists. Use --name {{}} to specify a new experiment.")
                self._refused = True
            else:
                self._open_log(a.log_path)
        # every rank leaves together: a master that returned alone would leave the others waiting in their next collective
        if broadcast_object(a, getattr(self, "_refused", False)):
            return False
        if self.master:
            for d in (a.checkpoint_path, a.tensorboard_path):
                if d:
                    os.makedirs(d, exist_ok=True)
        if a.resume == "latest":
            a.resume = self._find_latest()
        return True

    def _open_log(self, path):
        handler = logging.FileHandler(path)
        handler.setFormatter(logging.Formatter("%(asctime)s | %(levelname)s | %(message)s"))
        logging.getLogger().addHandler(handler)
        self._file_handler = handler

    def _find_latest(self):
        """`--resume latest` (reference main.py:138-170): with --save-most-recent the fixed name epoch_latest.pt, otherwise
        the newest checkpoint of this experiment; looked up on the master, broadcast so every rank resumes from one file."""
        a, found = self.args, None
        if self.master:
            if a.save_most_recent:
                cand = os.path.join(a.checkpoint_path, LATEST_CHECKPOINT_NAME)
                found = cand if os.path.exists(cand) else None
            else:
                found = get_latest_checkpoint(a.checkpoint_path)
            logging.info(f"Found latest resume checkpoint at {found}." if found
                         else f"No latest resume checkpoint found in {a.checkpoint_path}.")
        return broadcast_object(a, found)

    # ---- model, gradient averaging, optimizer ----------------------------------------------------------------------
    def build(self):
        a = self.args
        if isinstance(a.force_image_size, (tuple, list)) and len(a.force_image_size) == 1:
            a.force_image_size = a.force_image_size[0]
        random_seed(a.seed, 0)                       # same initial weights on every rank
        # EXTENSION: --siglip starts from open_clip's trainer values (the reference's main.py never sets a logit bias, so its
        # SigLipLoss would get none); the bias is then a parameter like logit_scale (no weight decay by its name)
        siglip_init = dict(init_logit_scale=math.log(10), init_logit_bias=-10.0) if getattr(a, "siglip", False) else {}
        self.core, self.pre_train, self.pre_val = create_model_and_transforms(
            a.model, a.pretrained, precision=a.precision, device=self.device, jit=a.torchscript,
            force_quick_gelu=a.force_quick_gelu, force_custom_text=a.force_custom_text,
            force_patch_dropout=a.force_patch_dropout, force_image_size=a.force_image_size,
            image_mean=a.image_mean, image_std=a.image_std, image_interpolation=a.image_interpolation,
            image_resize_mode=a.image_resize_mode, aug_cfg=a.aug_cfg, pretrained_image=a.pretrained_image, output_dict=True,
            **siglip_init)
        if distill_enabled(a):
            # the teacher: no DDP wrap, not in the optimizer, not checkpointed; it runs without a graph (train_one_epoch)
            self.dist_model = create_model(a.distill_model, a.distill_pretrained, device=self.device, precision=a.precision,
                                           output_dict=True)
        random_seed(a.seed, a.rank)
        if a.grad_checkpointing:
            self.core.set_grad_checkpointing()
        if self.master:
            logging.info(f"Model: {a.model}  params: {sum(p.numel() for p in self.core.parameters()):,}")
            with open(os.path.join(a.logs_dir, a.name, "params.txt"), "w") as f:
                f.writelines(f"{key}: {getattr(a, key)}\n" for key in sorted(vars(a)))
        self.model = self.core
        if a.distributed:
            if a.ddp_wrap:      # the reference's literal wrap (main.py:264-271); the towers' arenas are still reduced by our hooks
                kw = {"static_graph": True} if a.ddp_static_graph else {}
                self.model = torch.nn.parallel.DistributedDataParallel(self.core, device_ids=[self.device], **kw)
            else:
                wire = torch.bfloat16 if a.grad_comm_dtype == "bf16" else None
                self.grad_sync = GradSync(list(self.core.parameters()), a.world_size, grad_dtype=wire,
                                          shard_optimizer=a.shard_optimizer).attach(self.core)
        will_train = bool(a.train_data or a.dataset_type == "synthetic")
        if will_train:
            groups = param_groups(self.core.named_parameters(), a.wd)
            if self.grad_sync is not None and self.grad_sync.shard:
                self.optimizer = ShardedAdamW(groups, self.grad_sync, lr=a.lr, betas=(a.beta1, a.beta2), eps=a.eps)
            else:
                self.optimizer = FusedAdamW(groups, lr=a.lr, betas=(a.beta1, a.beta2), eps=a.eps)

    def restore(self):
        a = self.args
        if a.resume is None:
            return
        ckpt = torch.load(a.resume, map_location='cpu', weights_only=True)
        full = isinstance(ckpt, dict) and 'epoch' in ckpt        # train checkpoint vs bare state dict
        sd = ckpt["state_dict"] if full else ckpt
        if next(iter(sd)).startswith('module'):
            sd = {k[len('module.'):]: v for k, v in sd.items()}
        self.core.load_state_dict(sd)
        if full:
            self.start_epoch = ckpt["epoch"]
            if self.optimizer is not None:
                self.optimizer.load_state_dict(ckpt["optimizer"])
        logging.info(f"=> {'resuming' if full else 'loaded'} checkpoint '{a.resume}' (epoch {self.start_epoch})")

    # ---- data + schedule ---------------------------------------------------------------------------------------
    def load_data(self) -> bool:
        a = self.args
        self.data = get_data(a, (self.pre_train, self.pre_val), epoch=self.start_epoch, model=self.core)
        assert len(self.data), 'At least one train or eval dataset must be specified.'
        if 'train' in self.data and self.optimizer is not None:
            per_epoch = self.data["train"].dataloader.num_batches // a.accum_freq
            total = per_epoch * a.epochs
            if a.lr_scheduler == "cosine":
                self.scheduler = schedules.cosine_lr(self.optimizer, a.lr, a.warmup, total)
            elif a.lr_scheduler == "const":
                self.scheduler = schedules.const_lr(self.optimizer, a.lr, a.warmup, total)
            elif a.lr_scheduler == "const-cooldown":
                assert a.epochs_cooldown is not None, "Please specify the number of cooldown epochs for this lr schedule."
                self.scheduler = schedules.const_lr_cooldown(self.optimizer, a.lr, a.warmup, total, per_epoch * a.epochs_cooldown,
                                                             a.lr_cooldown_power, a.lr_cooldown_end)
            else:
                logging.error(f'Unknown scheduler, {a.lr_scheduler}. Available options are: cosine, const, const-cooldown.')
                return False
        if a.save_logs and a.tensorboard:
            from torch.utils import tensorboard          # ImportError here says what to install
            self.writer = tensorboard.SummaryWriter(a.tensorboard_path)
        return True

    # ---- epochs ------------------------------------------------------------------------------------------------
    def run(self):
        a = self.args
        if 'train' not in self.data:
            evaluate(self.model, self.data, self.start_epoch, a, tb_writer=self.writer)
            return
        loss = create_loss(a)
        has_eval = any(k in self.data for k in RETRIEVAL_SPLITS)   # the splits evaluate() implements; imagenet flags are refused at start-up
        for epoch in range(self.start_epoch, a.epochs):
            if self.master:
                logging.info(f'Start epoch {epoch}')
            train_one_epoch(self.model, self.data, loss, epoch, self.optimizer, None, self.scheduler, self.dist_model, a,
                            tb_writer=self.writer, grad_sync=self.grad_sync)
            if has_eval:
                evaluate(self.model, self.data, epoch + 1, a, tb_writer=self.writer)
            if hasattr(self.optimizer, "gather_state"):
                self.optimizer.gather_state()           # sharded moments -> whole, on every rank (a collective)
            if a.save_logs:
                self.save(epoch + 1)

    def save(self, done_epochs):
        """File names and dict keys of reference main.py:413-441."""
        a = self.args
        state = {"epoch": done_epochs, "name": a.name, "state_dict": self.core.state_dict(),
                 "optimizer": self.optimizer.state_dict()}
        periodic = a.save_frequency > 0 and done_epochs % a.save_frequency == 0
        if done_epochs == a.epochs or periodic:
            torch.save(state, os.path.join(a.checkpoint_path, f"epoch_{done_epochs}.pt"))
        if a.delete_previous_checkpoint:
            stale = os.path.join(a.checkpoint_path, f"epoch_{done_epochs - 1}.pt")
            if os.path.exists(stale):
                os.remove(stale)
        if a.save_most_recent:
            tmp = os.path.join(a.checkpoint_path, "tmp.pt")       # never leave a half-written epoch_latest.pt behind
            torch.save(state, tmp)
            os.replace(tmp, os.path.join(a.checkpoint_path, LATEST_CHECKPOINT_NAME))

    def close(self, clean: bool = True):
        """`clean` = the run ended without an exception.  Only then do the ranks meet in a barrier before the process group is
        destroyed: a rank that raised (out of memory, a data error) must not wait for ranks that sit in some other collective --
        it exits non-zero and the launcher tears the job down."""
        handler = getattr(self, "_file_handler", None)
        if handler is not None:
            logging.getLogger().removeHandler(handler)
            handler.close()
        if self.writer is not None:
            self.writer.close()
        if self.args.distributed and clean:
            torch.distributed.barrier()
            torch.distributed.destroy_process_group()


def main(args):
    run = _Run(args)
    clean = False
    try:
        if not run.open_experiment():
            clean = True               # every rank returns -1 together (the verdict is broadcast)
            return -1
        run.build()
        run.restore()
        if not run.load_data():
            clean = True
            return -1
        run.run()
        clean = True
    finally:
        run.close(clean)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
