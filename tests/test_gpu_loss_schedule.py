"""GPU checks of the loss-weight schedules: the backward under weights it was never run with.  The small KD model built by the
registry from the shipped KD config (tests/golden/kd_config.json; T = 2, 64 x 96 frames, B = 1, two targets, dropout as
configured, 256 points), seeds reset before every call.

  * a common power-of-two factor on all weights, set through a schedule, scales every loss and every gradient exactly: the root
    scale of the backward follows the weights (loss_schedule.weight_rel).  The same run without loss_weight_ref is measured, not
    judged: its largest relative gradient difference is printed (and written to the file S2D_LOSS_SCHEDULE_PARITY names;
    profiles/loss_schedule/parity.txt holds the figure of an MI355X run).
  * LossWeightSchedule.apply does nothing but set the weights: lockstep with a copy whose dict is set by hand from the simulator of
    tests/test_loss_schedule_cpu.py;
  * zero kd weights: exact zeros in the loss dict, the gradients of a run whose kd weights were zeroed by hand;
  * `python -m s2d_amd.train`: weight/* in metrics.json, a resumed run ends where the uninterrupted one does, default keys write
    nothing new.  Fresh child processes under a timeout."""
import hashlib
import json
import os
import shutil

import pytest
import torch

from tests.test_loss_schedule_cpu import MF, schedule_cfg, simulate, weight_dict

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KD_CFG = os.path.join(ROOT, "tests", "golden", "kd_config.json")
DEV = "cuda:0"
SMALL = ["INPUT.SAMPLING_FRAME_NUM", "2", MF + "TRAIN_NUM_POINTS", "256"]
T, H0, W0, N_GT = 2, 64, 96, 2


def _build(cfg):
    """the registry's model with the teacher a copy of the student whose class bias lets some queries pass the KD threshold"""
    from s2d_amd.modeling.meta_arch import META_ARCH_REGISTRY
    torch.manual_seed(0)
    model = META_ARCH_REGISTRY.get(cfg.MODEL.META_ARCHITECTURE).from_config(cfg).to(DEV)
    model.teacher.load_state_dict(model.student.state_dict())
    with torch.no_grad():
        model.teacher[1].predictor.class_embed.bias.copy_(torch.tensor([2.0, -2.0]))
    model.train()
    return model


def _seeded(model, seed=123):
    from s2d_amd import ops
    torch.manual_seed(seed); ops._DROP_CALLS[0] = 0
    model.criterion.seed = 0; model.criterion.matcher.seed = 0


@pytest.fixture(scope="module")
def clips():
    from tests.test_gpu_dropin import _clip_batch
    return [_clip_batch(T, H0, W0, N_GT, seed=5, B=1), _clip_batch(T, H0, W0, N_GT, seed=11, B=1)]


def _forward_backward(model, data):
    """one seeded forward_backward from empty gradients -> (loss dict, student gradients), clones"""
    from s2d_amd.modeling import TargetSet
    from s2d_amd.modeling.meta_arch import _gt_target_list
    for p in model.student.parameters():
        p.grad = None
    _seeded(model)
    images = model.preprocess(data)
    gt = TargetSet.from_list(_gt_target_list(data, T, images.shape[1], images.shape[2], model.device), device=model.device)
    losses = model.forward_backward(images, gt)
    torch.cuda.synchronize()
    return {k: v.clone() for k, v in losses.items()}, [p.grad.clone() for p in model.student.parameters()]


def test_power_of_two_weights_scale_losses_and_gradients_exactly(clips):
    from s2d_amd.loss_schedule import LossWeightSchedule
    f = 2.0 ** -7
    # linear, both minima 2^-7, step decay at 1: at iteration 1 the kd keys sit at their minimum (q = 0) and the supervised keys, still
    # at W0, are multiplied by SUPERVISED_MIN_WEIGHT -- every weight is W0 * 2^-7
    cfg = schedule_cfg("linear", 1, 0, -1, f, f, max_iter=8, extra=SMALL)
    model = _build(cfg)
    w0 = dict(model.criterion.weight_dict)
    assert not hasattr(model, "loss_weight_ref")
    l0, g0 = _forward_backward(model, clips[0])
    assert any(float(v) != 0.0 for v in l0.values()) and all(bool(torch.isfinite(g).all()) for g in g0)
    assert sum(bool(g.any()) for g in g0) > len(g0) // 2 and int(model.last["kd_count"].sum()) > 0
    sched = LossWeightSchedule(cfg, w0)
    wd = sched.apply(model, 1)
    assert wd == {k: v * f for k, v in w0.items()} and model.loss_weight_ref == 5.0
    l1, g1 = _forward_backward(model, clips[0])
    assert set(l1) == set(l0)
    for k in l0:
        assert torch.equal(l1[k], l0[k] * f), k
    for a, b in zip(g0, g1):
        assert torch.equal(b, a * f)
    # the same weights without the reference magnitude: the backward's operands sit 2^-7 lower.  A figure, not a bar.
    del model.loss_weight_ref
    l2, g2 = _forward_backward(model, clips[0])
    assert all(torch.equal(l2[k], l1[k]) for k in l1)
    rel = max(float((b - a * f).abs().max()) / float((a * f).abs().max()) for a, b in zip(g0, g2) if bool(a.any()))
    differ = sum(not torch.equal(b, a * f) for a, b in zip(g0, g2))
    line = (f"weights x 2^-7 without loss_weight_ref: max over parameters of max|g - 2^-7 g0| / max|2^-7 g0| = {rel:.3e}; "
            f"{differ} of {len(g0)} gradients differ" + ("" if differ else " (the two are equal at this size)"))
    print("loss_schedule parity:", line)
    if os.environ.get("S2D_LOSS_SCHEDULE_PARITY"):
        with open(os.environ["S2D_LOSS_SCHEDULE_PARITY"], "w") as fh:
            fh.write(line + "\n")
    model.criterion.weight_dict = w0


def test_apply_only_sets_the_weights(clips):
    from s2d_amd.engine import run_step
    from s2d_amd.loss_schedule import LossWeightSchedule
    from s2d_amd.optim import build_optimizer
    from s2d_amd.train import ema_momentum_at
    cfg = schedule_cfg("cosine", 2, 0, -1, 0.25, 0.5, max_iter=5, extra=SMALL + ["SOLVER.BASE_LR", "1e-4"])
    models = [_build(cfg) for _ in range(3)]                  # scheduled by apply(), by hand, constant
    opts = [build_optimizer(cfg, m) for m in models]
    w0 = dict(models[0].criterion.weight_dict)
    sched = LossWeightSchedule(cfg, w0)
    assert sched.active
    want = simulate(cfg, w0, 5)
    assert want[1] != w0 and want[2]["loss_mask"] < 0.25 * want[1]["loss_mask"] and want[3]["loss_mask"] > want[2]["loss_mask"]
    seen = [[], [], []]
    for it in range(5):
        data = clips[it % 2]
        for j, (m, o) in enumerate(zip(models, opts)):
            if j == 0:
                sched.apply(m, it)
            elif j == 1:
                m.criterion.weight_dict = dict(want[it])
                m.loss_weight_ref = max(abs(v) for v in w0.values())
            _seeded(m, 100 + it)
            losses = run_step(m, o, data, it, ema_momentum_at(cfg, it))
            seen[j].append({k: v.clone() for k, v in losses.items()})
    torch.cuda.synchronize()
    for it in range(5):
        a, b, c = (s[it] for s in seen)
        assert set(a) == set(b) == set(c)
        assert all(torch.equal(a[k], b[k]) for k in a), it
        assert all(bool(torch.isfinite(v)) for v in a.values())
        same = all(torch.equal(a[k], c[k]) for k in a)
        assert same == (it == 0), it                          # constant weights: the same step at 0, another loss dict from 1 on
    for name in ("student", "teacher"):
        pa, pb, pc = ([p.detach() for p in getattr(m, name).parameters()] for m in models)
        assert all(torch.equal(x, y) for x, y in zip(pa, pb)), name
        assert any(not torch.equal(x, y) for x, y in zip(pa, pc)), name
    assert models[2].criterion.weight_dict == w0 and not hasattr(models[2], "loss_weight_ref")


def test_zero_kd_weights_are_exact(clips):
    from s2d_amd.loss_schedule import LossWeightSchedule
    cfg = schedule_cfg("linear", 0, 0, -1, 0.0, 0.0, max_iter=8, extra=SMALL)
    model = _build(cfg)
    w0 = dict(model.criterion.weight_dict)
    sched = LossWeightSchedule(cfg, w0)
    wd = sched.apply(model, 1)                                # q = 0: the kd weights start at KD_MIN_WEIGHT = 0
    assert all(wd[k] == 0.0 for k in wd if "kd" in k) and all(wd[k] == w0[k] for k in wd if "kd" not in k)
    l1, g1 = _forward_backward(model, clips[1])
    assert all(float(l1[k]) == 0.0 for k in ("kd_loss_ce", "kd_loss_mask", "kd_loss_dice"))
    assert all(float(v) == 0.0 for k, v in l1.items() if "kd" in k)
    assert all(bool(torch.isfinite(v)) for v in l1.values()) and all(bool(torch.isfinite(g).all()) for g in g1)
    assert any(float(v) > 0.0 for v in l1.values()) and sum(bool(g.any()) for g in g1) > len(g1) // 2
    del model.loss_weight_ref
    model.criterion.weight_dict = {k: (0.0 if "kd" in k else v) for k, v in w0.items()}
    l2, g2 = _forward_backward(model, clips[1])
    assert all(torch.equal(l1[k], l2[k]) for k in l1)
    assert all(torch.equal(a, b) for a, b in zip(g1, g2))


# ------------------------------------------------------------------------------------------------------------ the driver
@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    from tests.test_gpu_train_driver import _write_dataset
    root = str(tmp_path_factory.mktemp("ytvis_sched"))
    return root, _write_dataset(root)


@pytest.fixture(scope="module")
def checkpoint(tmp_path_factory):
    from s2d_amd.checkpoint import kd_to_plain
    from s2d_amd.config import load_config
    from s2d_amd.modeling.meta_arch import META_ARCH_REGISTRY
    cfg = load_config(KD_CFG)
    torch.manual_seed(0)
    model = META_ARCH_REGISTRY.get(cfg.MODEL.META_ARCHITECTURE).from_config(cfg)
    path = str(tmp_path_factory.mktemp("init") / "init.pth")
    torch.save({"model": kd_to_plain({k: v.detach().cpu() for k, v in model.state_dict().items()})}, path)
    return path


DRIVER_OPTS = ["INPUT.MIN_SIZE_TRAIN", "(64,)", "SOLVER.IMS_PER_BATCH", "2", "SOLVER.BASE_LR", "1e-4", "SOLVER.CHECKPOINT_PERIOD", "2",
               "SEED", "1", "SOLVER.MAX_ITER", "4", MF + "TRAIN_NUM_POINTS", "256"]
SCHEDULE_OPTS = [MF + "KD_WEIGHT_SCHEDULER", "linear", MF + "LOSS_WEIGHT_DECAY_STEP", "2"]


def _train(dataset, checkpoint, out, opts, extra=()):
    from tests.test_gpu_train_driver import _run
    root, path = dataset
    return _run("s2d_amd.train", ["--config-file", KD_CFG, "--train-json", path, "--image-root", root, "--output-dir", str(out),
                                  "--weights", checkpoint, "--threads", "4"] + list(extra) + DRIVER_OPTS + list(opts), timeout=600)


def _student_digest(path):
    ck = torch.load(path, map_location="cpu", weights_only=True)["model"]
    h = hashlib.sha1()
    for k in sorted(ck):
        if k.startswith("student."):
            h.update(ck[k].numpy().tobytes())
    return h.hexdigest()


def test_driver_logs_the_weights_and_resumes_onto_the_same_run(dataset, checkpoint, tmp_path):
    from s2d_amd.config import load_config
    out = tmp_path / "full"
    lines = _train(dataset, checkpoint, out, SCHEDULE_OPTS)
    cfg = load_config(KD_CFG, DRIVER_OPTS + SCHEDULE_OPTS)
    mf = cfg.MODEL.MASK_FORMER
    w0 = weight_dict(mf.DEC_LAYERS, {"loss_ce": mf.CLASS_WEIGHT, "loss_mask": mf.MASK_WEIGHT, "loss_dice": mf.DICE_WEIGHT,
                                     "kd_loss_ce": mf.KD_CLASS_WEIGHT, "kd_loss_mask": mf.KD_MASK_WEIGHT, "kd_loss_dice": mf.KD_DICE_WEIGHT})
    want = simulate(cfg, w0, 4)
    assert want[3] != want[2] != want[1] != w0
    start = [l for l in lines if "loss_weight_scheduler" in l]
    assert start == [{"loss_weight_scheduler": "linear", "start": 0, "end": 4, "D": 2, "supervised_min_weight": mf.SUPERVISED_MIN_WEIGHT,
                      "kd_min_weight": mf.KD_MIN_WEIGHT}]
    recs = [json.loads(l) for l in open(out / "metrics.json")]
    assert [r["iteration"] for r in recs] == [3]
    base = ("loss_ce", "loss_mask", "loss_dice", "kd_loss_ce", "kd_loss_mask", "kd_loss_dice")
    assert {k: v for k, v in recs[0].items() if k.startswith("weight/")} == {f"weight/{k}": want[3][k] for k in base}
    # resumed after iteration 1: iterations 2 and 3 with the weights (and the seeds) of the uninterrupted run
    assert (out / "model_0000001.pth").exists() and (out / "model_final.pth").exists()
    res = tmp_path / "resumed"
    shutil.copytree(out, res)
    (res / "last_checkpoint").write_text("model_0000001.pth")
    os.remove(res / "metrics.json"); os.remove(res / "model_final.pth"); os.remove(res / "model_0000003.pth")
    lines = _train(dataset, checkpoint, res, SCHEDULE_OPTS, extra=["--resume"])
    assert lines[0]["start_iter"] == 2 and [l for l in lines if "iterations" in l][-1]["iterations"] == 2
    again = [json.loads(l) for l in open(res / "metrics.json")]
    assert {k: v for k, v in again[0].items() if k.startswith("weight/")} == {f"weight/{k}": want[3][k] for k in base}
    assert _student_digest(res / "model_final.pth") == _student_digest(out / "model_final.pth")
    # default keys: no schedule line, no weight/* key
    plain = tmp_path / "plain"
    lines = _train(dataset, checkpoint, plain, [])
    assert not [l for l in lines if "loss_weight_scheduler" in l]
    recs = [json.loads(l) for l in open(plain / "metrics.json")]
    assert [r["iteration"] for r in recs] == [3] and not [k for k in recs[0] if k.startswith("weight/")]
    assert _student_digest(plain / "model_final.pth") != _student_digest(out / "model_final.pth")
