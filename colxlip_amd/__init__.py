"""colxlip_amd — MI355X-native CLIP train step behind the reference's package API
(reference src/colxlip/__init__.py:1-5; the same names are importable as `colxlip`, see ../colxlip/__init__.py)."""
from .factory import create_model, create_model_and_transforms, create_loss, get_tokenizer
from .factory import list_models, add_model_config, get_model_config, load_checkpoint, download_weights_from_hf
from .loss import ClipLoss, ColClipLoss, DistillClipLoss, SigLipLoss, compute_colbert_similarity, gather_features
from .model import CLIP, ColXLIP, CLIPTextCfg, CLIPVisionCfg, get_cast_dtype, get_input_dtype
from .model import convert_weights_to_lp, convert_weights_to_fp16, trace_model
from .model import get_model_tokenize_cfg, get_model_preprocess_cfg, set_model_preprocess_cfg
from . import ops

__version__ = "0.3.0"


def __getattr__(name):
    # resolved on first use: `python -m colxlip_amd.search` must not find its own module imported already
    if name == "LateInteractionIndex":
        from .search import LateInteractionIndex
        return LateInteractionIndex
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
