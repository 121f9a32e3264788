"""Checkpoint loading with the reference's key conversions (model_training/mask2former_video/engine/checkpoint.py:157-176,
193-286):

* a plain checkpoint (backbone.* / sem_seg_head.*) loaded into a KD model fans out to student.{0,1}.* AND teacher.{0,1}.*;
* a KD checkpoint (student.* / teacher.*) loaded into a VideoMaskFormer keeps the TEACHER: teacher.0.* -> backbone.*,
  teacher.1.* -> sem_seg_head.* (everything else is dropped, as there).

Tensors whose shape differs from the model's are skipped with a warning, as detectron2's checkpointer does.  The library's
modules cache packed / pre-split images of their weights; those are dropped here, so weights loaded into a model that has
already run a forward take effect.

detectron2 `.pkl` files ({"model": {name: ndarray}, "__author__": ..., ["matching_heuristics": True]}, pickled with
encoding="latin1") are read through a restricted unpickler that admits numpy arrays, numpy scalars and plain containers only.
Exact detectron2 model names go through the same conversions as a .pth; the backbone-only ImageNet files
(torchvision-converted names stem.* / res2.* ... res5.*) are mapped onto backbone.* (student.0.* and teacher.0.* in a KD
model).  detectron2's general suffix-matching heuristic (`matching_heuristics`) is not implemented: names that match neither
form are reported as unexpected, like any other unmatched key."""
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


_BACKBONE_TOP = ("stem.", "res2.", "res3.", "res4.", "res5.")

# what a detectron2 .pkl may contain: ndarray reconstruction and dtypes, numpy scalars, plain containers
_PKL_ALLOWED = {
    ("numpy.core.multiarray", "_reconstruct"), ("numpy._core.multiarray", "_reconstruct"),
    ("numpy.core.multiarray", "scalar"), ("numpy._core.multiarray", "scalar"),
    ("numpy", "ndarray"), ("numpy", "dtype"),
    ("collections", "OrderedDict"), ("builtins", "dict"), ("builtins", "list"), ("builtins", "tuple"), ("builtins", "set"),
}


class _ArrayUnpickler(pickle.Unpickler):
    """refuses every global outside _PKL_ALLOWED (a .pkl could otherwise run arbitrary code when loaded)"""

    def find_class(self, module, name):
        if (module, name) in _PKL_ALLOWED:
            return super().find_class(module, name)
        raise pickle.UnpicklingError(f"refusing {module}.{name} in a .pkl checkpoint: only numpy arrays, numpy scalars and plain "
                                     "containers are read")


def read_pkl(path):
    """a detectron2 .pkl -> {name: tensor}.  Backbone-only files (every name under stem. / res2. ... res5.) get the backbone.
    prefix so that the plain / KD conversions place them."""
    with open(path, "rb") as f:
        data = _ArrayUnpickler(f, encoding="latin1").load()
    sd = data["model"] if isinstance(data, dict) and "model" in data else data
    if not isinstance(sd, dict):
        raise pickle.UnpicklingError(f"{path}: expected a dict of arrays, found {type(sd).__name__}")
    out = {}
    for k, v in sd.items():
        if not isinstance(v, (np.ndarray, np.generic)):
            raise pickle.UnpicklingError(f"{path}: entry {k!r} is a {type(v).__name__}, not a numpy array")
        out[k] = torch.from_numpy(np.array(v))
    if out and all(k.startswith(_BACKBONE_TOP) for k in out):
        out = {"backbone." + k: v for k, v in out.items()}
    return out


def read_state_dict(path):
    """a torch .pth or a detectron2 .pkl -> its state dict (the "model" entry when there is one)"""
    if path.endswith(".pkl"):
        return read_pkl(path)
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
    from .weight_cache import PackedSlot, clear_weight_cache
    clear_weight_cache()
    for m in model.modules():
        for slot in vars(m).values():
            if isinstance(slot, PackedSlot):
                slot.reset()


def load_checkpoint(model, path_or_state_dict):
    """load a .pth / .pkl (or a state dict) into `model` -> {"missing": [...], "unexpected": [...], "mismatched": [(key, ckpt shape,
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
