"""Class-aware configurations (SEM_SEG_HEAD.NUM_CLASSES > 1) build through the registry, and detectron2 .pkl checkpoints load.
No GPU needed."""
import os
import pickle

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIG = os.path.join(ROOT, "tests", "golden", "kd_config.json")


def class_config(meta_arch, num_classes, small=False, extra=()):
    from s2d_amd.config import load_config
    opts = ["MODEL.META_ARCHITECTURE", meta_arch, "MODEL.SEM_SEG_HEAD.NUM_CLASSES", str(num_classes),
            "MODEL.MASK_FORMER.CLASS_WEIGHT", "2.0"]
    if small:
        opts += ["MODEL.MASK_FORMER.NUM_OBJECT_QUERIES", "12", "MODEL.MASK_FORMER.DEC_LAYERS", "3",
                 "MODEL.MASK_FORMER.TRAIN_NUM_POINTS", "256", "INPUT.SAMPLING_FRAME_NUM", "2",
                 "MODEL.MASK_FORMER.NUM_PREDICTIONS_DISTILLATION", "24", "MODEL.MASK_FORMER.SCORE_THRESHOLD_DISTILLATION", "0.3",
                 "MODEL.MASK_FORMER.DROPOUT", "0.0"]
    return load_config(CONFIG, opts + list(extra))


def build_model(meta_arch, num_classes, small=False, extra=()):
    from s2d_amd.modeling.meta_arch import META_ARCH_REGISTRY
    cfg = class_config(meta_arch, num_classes, small, extra)
    return META_ARCH_REGISTRY.get(cfg.MODEL.META_ARCHITECTURE).from_config(cfg)


@pytest.mark.parametrize("num_classes", [40, 1203])
@pytest.mark.parametrize("meta_arch", ["KDVideoMaskFormer", "VideoMaskFormer"])
def test_class_aware_configs_build(meta_arch, num_classes):
    model = build_model(meta_arch, num_classes, small=True)
    heads = [model.student[1], model.teacher[1]] if meta_arch == "KDVideoMaskFormer" else [model.sem_seg_head]
    for h in heads:
        assert h.num_classes == num_classes
        assert tuple(h.predictor.class_embed.weight.shape) == (num_classes + 1, 256)
    crit = model.criterion
    assert crit.num_classes == num_classes
    assert tuple(crit.empty_weight.shape) == (num_classes + 1,)
    assert float(crit.empty_weight[-1]) == pytest.approx(0.1) and float(crit.empty_weight[:-1].min()) == 1.0
    wd = crit.weight_dict
    assert wd["loss_ce"] == 2.0 and wd["loss_ce_0"] == 2.0 and wd["loss_mask"] == 5.0 and "loss_ce_2" not in wd
    if meta_arch == "KDVideoMaskFormer":
        assert model._kd_slots(12) == 24                   # min(NUM_PREDICTIONS_DISTILLATION, Q * C): one query, several labels


def test_full_size_class_aware_config_builds():
    model = build_model("KDVideoMaskFormer", 40)
    assert model.student[1].predictor.class_embed.out_features == 41
    assert model._kd_slots(100) == 100


@pytest.mark.parametrize("extra,what", [
    (["MODEL.SEM_SEG_HEAD.NUM_CLASSES", "0"], "NUM_CLASSES"),
    (["MODEL.MASK_FORMER.NUM_OBJECT_QUERIES", "200"], "NUM_OBJECT_QUERIES"),
    (["MODEL.MASK_FORMER.NUM_PREDICTIONS_DISTILLATION", "300"], "NUM_PREDICTIONS_DISTILLATION"),
])
def test_unsupported_configs_are_refused_at_from_config(extra, what):
    with pytest.raises(ValueError, match=what):
        build_model("KDVideoMaskFormer", 40, extra=extra)


def test_class_agnostic_config_unchanged():
    model = build_model("KDVideoMaskFormer", 1, small=True)
    assert model.student[1].predictor.class_embed.out_features == 2
    assert model._kd_slots(12) == 12


def _write_pkl(path, sd, **extra):
    with open(path, "wb") as f:
        pickle.dump({"model": {k: v.numpy() for k, v in sd.items()}, "__author__": "test", **extra}, f)


def test_pkl_detectron2_names_load_identically(tmp_path):
    from s2d_amd.checkpoint import load_checkpoint
    from s2d_amd.checkpoint import kd_to_plain
    src = build_model("VideoMaskFormer", 40, small=True)
    with torch.no_grad():
        for i, p in enumerate(src.parameters()):
            p.copy_(torch.randn(p.shape, generator=torch.Generator().manual_seed(i)))
    sd = src.state_dict()
    _write_pkl(tmp_path / "m.pkl", sd, matching_heuristics=True)
    dst = build_model("VideoMaskFormer", 40, small=True)
    info = load_checkpoint(dst, str(tmp_path / "m.pkl"))
    assert info["missing"] == [] and info["unexpected"] == [] and info["mismatched"] == []
    for k, v in dst.state_dict().items():
        assert torch.equal(v, sd[k]), k
    # the same plain checkpoint into a KD model fans out to student and teacher
    kd = build_model("KDVideoMaskFormer", 40, small=True)
    info = load_checkpoint(kd, str(tmp_path / "m.pkl"))
    assert all(k.startswith("criterion.") for k in info["missing"]) and info["mismatched"] == []
    back = kd_to_plain(kd.state_dict())
    for k, v in sd.items():
        if k.startswith("criterion."):
            continue
        assert torch.equal(back[k], v), k
        assert torch.equal(kd.state_dict()[k.replace("sem_seg_head.", "student.1.").replace("backbone.", "student.0.")], v)


def test_pkl_backbone_only_names_map_onto_backbones(tmp_path):
    from s2d_amd.checkpoint import load_checkpoint
    from s2d_amd.modeling.backbone import ResNet50
    r = ResNet50()
    with torch.no_grad():
        for i, p in enumerate(r.parameters()):
            p.copy_(torch.randn(p.shape, generator=torch.Generator().manual_seed(100 + i)))
    sd = r.state_dict()
    assert all(k.startswith(("stem.", "res2.", "res3.", "res4.", "res5.")) for k in sd)
    _write_pkl(tmp_path / "R-50.pkl", sd)
    kd = build_model("KDVideoMaskFormer", 40, small=True)
    info = load_checkpoint(kd, str(tmp_path / "R-50.pkl"))
    assert info["unexpected"] == [] and info["mismatched"] == []
    assert all(k.startswith(("student.1.", "teacher.1.", "criterion.")) for k in info["missing"])
    own = kd.state_dict()
    for k, v in sd.items():
        assert torch.equal(own["student.0." + k], v) and torch.equal(own["teacher.0." + k], v), k
    vm = build_model("VideoMaskFormer", 40, small=True)
    load_checkpoint(vm, str(tmp_path / "R-50.pkl"))
    for k, v in sd.items():
        assert torch.equal(vm.state_dict()["backbone." + k], v), k


class _Payload:
    pass


def test_pkl_with_a_non_array_object_is_refused(tmp_path):
    from s2d_amd.checkpoint import read_state_dict
    with open(tmp_path / "bad.pkl", "wb") as f:
        pickle.dump({"model": {"stem.conv1.weight": np.zeros((2, 2), np.float32), "x": _Payload()}}, f)
    with pytest.raises(pickle.UnpicklingError, match="refusing"):
        read_state_dict(str(tmp_path / "bad.pkl"))
    with open(tmp_path / "bad2.pkl", "wb") as f:
        pickle.dump({"model": {"stem.conv1.weight": "not an array"}}, f)
    with pytest.raises(pickle.UnpicklingError, match="not a numpy array"):
        read_state_dict(str(tmp_path / "bad2.pkl"))


def test_new_entry_points_are_declared():
    from s2d_amd._lib import parse_header
    protos = parse_header()
    for name in ("s2d_class_loss_c_f32", "s2d_class_loss_backward_c_f32", "s2d_matcher_cost_c_f32", "s2d_matcher_c_workspace_floats",
                 "s2d_kd_targets_c_u8", "s2d_kd_targets_c_workspace_bytes", "s2d_infer_select_c_f32",
                 "s2d_infer_select_c_workspace_bytes"):
        assert name in protos
