"""Checkpoint loading with the reference's key conversions (model_training/mask2former_video/engine/checkpoint.py:157-176,
193-286):

* a plain checkpoint (backbone.* / sem_seg_head.*) loaded into a KD model fans out to student.{0,1}.* AND teacher.{0,1}.*;
* a KD checkpoint (student.* / teacher.*) loaded into a VideoMaskFormer keeps the TEACHER: teacher.0.* -> backbone.*,
  teacher.1.* -> sem_seg_head.* (everything else is dropped, as there).

Tensors whose shape differs from the model's are skipped with a warning, as detectron2's checkpointer does.  The library's
modules cache packed / pre-split images of their weights; those are dropped here, so weights loaded into a model that has
already run a forward take effect.  `.pkl` model-zoo files are not read."""
import logging
import pickle

import numpy as np
import torch

_log = logging.getLogger(__name__)
_KD = ("student.", "teacher.")


def plain_to_kd(sd):
    """backbone.* / sem_seg_head.* -> student.{0,1}.* and teacher.{0,1}.* (other keys dropped)"""
    out = {}
    for k, v in sd.items():
        if k.startswith("backbone."):
            out[k.replace("backbone.", "student.0.")] = v
            out[k.replace("backbone.", "teacher.0.")] = v
        elif k.startswith("sem_seg_head."):
            out[k.replace("sem_seg_head.", "student.1.")] = v
            out[k.replace("sem_seg_head.", "teacher.1.")] = v
    return out


def kd_to_plain(sd):
    """teacher.0.* -> backbone.*, teacher.1.* -> sem_seg_head.* (other keys dropped)"""
    out = {}
    for k, v in sd.items():
        if k.startswith("teacher.0."):
            out[k.replace("teacher.0.", "backbone.", 1)] = v
        elif k.startswith("teacher.1."):
            out[k.replace("teacher.1.", "sem_seg_head.", 1)] = v
    return out


def convert_state_dict(sd, model_keys):
    """apply the conversion the pair (checkpoint keys, model keys) calls for"""
    model_kd = any(k.startswith(_KD) for k in model_keys)
    ckpt_kd = any(k.startswith(_KD) for k in sd)
    if model_kd and not ckpt_kd:
        return plain_to_kd(sd)
    if ckpt_kd and not model_kd:
        return kd_to_plain(sd)
    return dict(sd)


def read_state_dict(path):
    """a torch .pth -> its state dict (the "model" entry when there is one)"""
    if path.endswith(".pkl"):
        raise NotImplementedError(".pkl model-zoo checkpoints are not supported: convert them to a torch .pth")
    try:
        ckpt = torch.load(path, map_location="cpu", weights_only=True)
    except pickle.UnpicklingError:
        # detectron2 checkpoints also hold trainer / scheduler state that the restricted unpickler refuses
        _log.warning("%s holds more than tensors; loading it with the full unpickler (trusted files only)", path)
        ckpt = torch.load(path, map_location="cpu", weights_only=False)
    sd = ckpt["model"] if isinstance(ckpt, dict) and "model" in ckpt else ckpt
    return {k: torch.from_numpy(np.asarray(v)) if not isinstance(v, torch.Tensor) else v for k, v in sd.items()}


def invalidate_weight_caches(model):
    """drop every packed / pre-split weight image the library keeps for `model` (they are rebuilt at the next forward)"""
    from . import ops
    ops.clear_weight_cache()
    for m in model.modules():
        for attr in ("_packed", "_fold", "_ws", "_kv_cache"):
            if getattr(m, attr, None) is not None:
                setattr(m, attr, None)


def load_checkpoint(model, path_or_state_dict):
    """load a .pth (or a state dict) into `model` -> {"missing": [...], "unexpected": [...], "mismatched": [(key, ckpt shape,
    model shape)]}"""
    sd = path_or_state_dict if isinstance(path_or_state_dict, dict) else read_state_dict(path_or_state_dict)
    own = model.state_dict()
    sd = convert_state_dict(sd, own.keys())
    mismatched, keep = [], {}
    for k, v in sd.items():
        if k in own and tuple(v.shape) != tuple(own[k].shape):
            _log.warning("skip %s: checkpoint shape %s, model shape %s", k, tuple(v.shape), tuple(own[k].shape))
            mismatched.append((k, tuple(v.shape), tuple(own[k].shape)))
            continue
        keep[k] = v
    res = model.load_state_dict(keep, strict=False)
    invalidate_weight_caches(model)
    missing = list(res.missing_keys) + [k for k, _, _ in mismatched]
    if missing:
        _log.warning("keys not loaded: %d (%s ...)", len(missing), ", ".join(missing[:5]))
    if res.unexpected_keys:
        _log.warning("unexpected keys: %d (%s ...)", len(res.unexpected_keys), ", ".join(res.unexpected_keys[:5]))
    return {"missing": missing, "unexpected": list(res.unexpected_keys), "mismatched": mismatched}


def evaluated_prefixes(model):
    """state-dict prefixes of the network the eval branch runs: teacher (or student with TEST.EVAL_STUDENT) of a KD model,
    backbone + head of a VideoMaskFormer"""
    if hasattr(model, "teacher"):
        return ("student.",) if getattr(model, "eval_student", False) else ("teacher.",)
    return ("backbone.", "sem_seg_head.")
