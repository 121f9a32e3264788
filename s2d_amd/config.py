"""Configs without detectron2: `load_config(path, opts)` reads a yaml of the reference's configs/ (PyYAML), resolves its `_BASE_`
chain relative to each file, applies `KEY VALUE` overrides and returns the attribute namespace that the `from_config` methods
and the test loader read (cfg.MODEL.MASK_FORMER.NHEADS, ...).

Values are decoded as yacs decodes them (a string that is a Python literal, e.g. "(360, 480)", becomes that literal).  Keys the
yamls may omit take the defaults of detectron2's get_cfg() with add_maskformer2_config / add_maskformer2_video_config
(mask2former/config.py, mask2former_video/config.py) for the keys this library reads.  A yaml may add keys the defaults do not
list; an override of a key that exists nowhere is an error."""
import ast
import copy
import os
from types import SimpleNamespace

import yaml

DEFAULTS = {
    "MODEL": {
        "META_ARCHITECTURE": "GeneralizedRCNN",
        "WEIGHTS": "",
        "PIXEL_MEAN": [103.53, 116.28, 123.675],
        "PIXEL_STD": [1.0, 1.0, 1.0],
        "BACKBONE": {"NAME": "build_resnet_backbone", "FREEZE_AT": 2},
        "SEM_SEG_HEAD": {"NAME": "SemSegFPNHead", "NUM_CLASSES": 54, "CONVS_DIM": 128, "MASK_DIM": 256,
                         "TRANSFORMER_ENC_LAYERS": 0, "PIXEL_DECODER_NAME": "BasePixelDecoder", "NORM": "GN",
                         "IGNORE_VALUE": 255, "COMMON_STRIDE": 4, "LOSS_WEIGHT": 1.0,
                         "DEFORMABLE_TRANSFORMER_ENCODER_IN_FEATURES": ["res3", "res4", "res5"],
                         "DEFORMABLE_TRANSFORMER_ENCODER_N_POINTS": 4, "DEFORMABLE_TRANSFORMER_ENCODER_N_HEADS": 8},
        "MASK_FORMER": {
            "DEEP_SUPERVISION": True, "NO_OBJECT_WEIGHT": 0.1, "CLASS_WEIGHT": 1.0, "DICE_WEIGHT": 1.0, "MASK_WEIGHT": 20.0,
            "NHEADS": 8, "DROPOUT": 0.1, "DIM_FEEDFORWARD": 2048, "ENC_LAYERS": 0, "DEC_LAYERS": 6, "PRE_NORM": False,
            "HIDDEN_DIM": 256, "NUM_OBJECT_QUERIES": 100, "TRANSFORMER_IN_FEATURE": "res5", "ENFORCE_INPUT_PROJ": False,
            "SIZE_DIVISIBILITY": 32, "TRANSFORMER_DECODER_NAME": "MultiScaleMaskedTransformerDecoder",
            "TRAIN_NUM_POINTS": 112 * 112, "OVERSAMPLE_RATIO": 3.0, "IMPORTANCE_SAMPLE_RATIO": 0.75,
            "LOSS_STRATEGY": "full", "NUM_PREDICTIONS_DISTILLATION": 100, "SCORE_THRESHOLD_DISTILLATION": 0.75,
            "KD_CLASS_WEIGHT": 0.0, "KD_MASK_WEIGHT": 5.0, "KD_DICE_WEIGHT": 5.0, "DETACH_CLS": False,
            "SPARSE_CLASS_WEIGHT": 0.0, "ENTROPY_WEIGHT": 0.0, "MASK_DROPLOSS": False, "LABEL_DROPLOSS": False,
            "NO_CLASS_MATCH": False, "DISTILLATION_NMS": False, "DISTILLATION_LOSS_STRATEGY": "masks-only",
            "EMA_MOMENTUM": 0.999, "EMA_MOMENTUM_SCHEDULE": False, "EMA_MOMENTUM_END": 0.999, "EMA_MOMENTUM_UNTIL_STEP": 10000,
            # the loss-weight schedules of the reference trainer (loss_schedule.py)
            "LOSS_WEIGHT_DECAY_STEP": 0.0, "KD_WEIGHT_SCHEDULER": "constant", "DECAY_ONLY_SUPERVISED_LOSS": False,
            "DECAY_ONLY_KD_LOSS": False, "SUPERVISED_MIN_WEIGHT": 0.0, "KD_MIN_WEIGHT": 0.0, "KD_WEIGHT_DECAY_START": 0.0,
            "KD_WEIGHT_DECAY_END": -1.0,
            "TEST": {"SEMANTIC_ON": True, "INSTANCE_ON": False, "PANOPTIC_ON": False, "OBJECT_MASK_THRESHOLD": 0.0,
                     "OVERLAP_THRESHOLD": 0.0, "SEM_SEG_POSTPROCESSING_BEFORE_INFERENCE": False, "USE_NMS": False,
                     "NMS_THRESH": 0.6, "NUM_PREDICTIONS": 10, "EVAL_STUDENT": False,
                     # this library's own keys (no reference counterpart): windowed inference of long videos, DESIGN.md section 1
                     "WINDOW_INFERENCE": False, "WINDOW_SIZE": 0, "WINDOW_OVERLAP": 0},
        },
    },
    "INPUT": {
        "MIN_SIZE_TRAIN": (800,), "MAX_SIZE_TRAIN": 1333, "MIN_SIZE_TRAIN_SAMPLING": "choice", "MIN_SIZE_TEST": 800,
        "MAX_SIZE_TEST": 1333, "RANDOM_FLIP": "horizontal", "FORMAT": "BGR",
        "CROP": {"ENABLED": False, "TYPE": "relative_range", "SIZE": [0.9, 0.9]},
        "SAMPLING_FRAME_NUM": 2, "SAMPLING_FRAME_RANGE": 20, "SAMPLING_FRAME_SHUFFLE": False, "AUGMENTATIONS": [],
        "DENSE_ANNOTATION_SELECTION": True, "DISENTANGLE_DISTILLATION_LOADER": False, "DISTILLATION_DENSE_ANNOTATION_SELECTION": True,
    },
    "DATASETS": {"TRAIN": (), "TEST": ()},
    "DATALOADER": {"NUM_WORKERS": 4, "ASPECT_RATIO_GROUPING": True, "FILTER_EMPTY_ANNOTATIONS": True, "COPY_PASTE": False,
                   "COPY_PASTE_RATE": 0.0, "COPY_PASTE_RANDOM_NUM": True, "VISUALIZE_COPY_PASTE": False, "COPY_PASTE_MIN_RATIO": 0.5, "COPY_PASTE_MAX_RATIO": 1.0,
                   "COPY_PASTE_DENSIFY_SPARSE": False},
    # the solver keys of detectron2's get_cfg() + add_maskformer2_config that the optimizer, the LR scheduler and the training
    # driver read
    "SOLVER": {"ACCUM_ITER": 1, "OPTIMIZER": "ADAMW", "BASE_LR": 0.001, "MAX_ITER": 40000, "STEPS": (30000,),
               "WEIGHT_DECAY": 0.0001, "WEIGHT_DECAY_NORM": 0.0, "WEIGHT_DECAY_EMBED": 0.0, "BACKBONE_MULTIPLIER": 0.1,
               "LR_SCHEDULER_NAME": "WarmupMultiStepLR", "GAMMA": 0.1, "WARMUP_FACTOR": 0.001, "WARMUP_ITERS": 1000,
               "WARMUP_METHOD": "linear", "POLY_LR_POWER": 0.9, "POLY_LR_CONSTANT_ENDING": 0.0, "CHECKPOINT_PERIOD": 5000,
               "IMS_PER_BATCH": 16,
               "CLIP_GRADIENTS": {"ENABLED": False, "CLIP_TYPE": "value", "CLIP_VALUE": 1.0, "NORM_TYPE": 2.0},
               "AMP": {"ENABLED": False}},
    "TEST": {"EVAL_PERIOD": 0},
    "SEED": -1,
    "OUTPUT_DIR": "./output",
}


def _decode(v):
    """yacs _decode_cfg_value: strings that are Python literals become them, lists / dicts are decoded element-wise"""
    if isinstance(v, dict):
        return {k: _decode(x) for k, x in v.items()}
    if isinstance(v, list):
        return [_decode(x) for x in v]
    if isinstance(v, str):
        try:
            return ast.literal_eval(v)
        except (ValueError, SyntaxError):
            return v
    return v


def _merge(dst, src):
    for k, v in src.items():
        if isinstance(v, dict) and isinstance(dst.get(k), dict):
            _merge(dst[k], v)
        else:
            dst[k] = copy.deepcopy(v)
    return dst


def _read(path, depth=0):
    if depth > 16:
        raise ValueError(f"_BASE_ chain too deep at {path}")
    with open(path) as fh:
        doc = yaml.safe_load(fh) or {}
    base = doc.pop("_BASE_", None)
    out = {}
    if base is not None:
        bp = base if os.path.isabs(base) else os.path.join(os.path.dirname(os.path.abspath(path)), base)
        out = _read(bp, depth + 1)
    return _merge(out, _decode(doc))


def _ns(d):
    return SimpleNamespace(**{k: _ns(v) if isinstance(v, dict) else v for k, v in d.items()})


def to_dict(cfg):
    """namespace from load_config -> plain nested dict"""
    return {k: to_dict(v) if isinstance(v, SimpleNamespace) else v for k, v in vars(cfg).items()}


def load_config(path, opts=()):
    """yaml (or JSON) config with its _BASE_ chain + overrides ["KEY.PATH", "VALUE", ...] -> nested SimpleNamespace"""
    cfg = _merge(copy.deepcopy(DEFAULTS), _read(path))
    opts = list(opts)
    if len(opts) % 2:
        raise ValueError(f"overrides come in KEY VALUE pairs, got {opts}")
    for key, val in zip(opts[0::2], opts[1::2]):
        node, parts = cfg, key.split(".")
        for p in parts[:-1]:
            if not isinstance(node.get(p), dict):
                raise KeyError(f"unknown config key {key}")
            node = node[p]
        if parts[-1] not in node or isinstance(node[parts[-1]], dict):
            raise KeyError(f"unknown config key {key}")
        node[parts[-1]] = _decode(val)
    return _ns(cfg)
