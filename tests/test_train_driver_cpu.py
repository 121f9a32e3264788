"""CPU checks of the training driver's host side: LR schedulers, config defaults the driver and build_optimizer read, the YTVIS
training dataset, the sampler (ranks, aspect buckets, resume), the sampling functions with explicit generators, the checkpoint
schedule and the CLI rejections."""
import json
import math
import os
import random

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
KD_CFG = os.path.join(HERE, "golden", "kd_config.json")


# ---------------------------------------------------------------------------------------------------------------- schedulers
class _Opt:
    def __init__(self, lrs):
        self.param_groups = [{"lr": lr, "params": []} for lr in lrs]


def _cfg(**solver):
    from s2d_amd.config import load_config
    opts = []
    for k, v in solver.items():
        opts += [f"SOLVER.{k}", repr(v)]
    return load_config(KD_CFG, opts)


def _lrs(cfg, iters, lrs=(1.0, 0.1)):
    from s2d_amd.solver import build_lr_scheduler
    opt = _Opt(lrs)
    sch = build_lr_scheduler(cfg, opt)
    out = {}
    for it in range(max(iters) + 1):
        if it in iters:
            out[it] = [g["lr"] for g in opt.param_groups]
        sch.step()
    return out


def test_multistep_without_warmup():
    cfg = _cfg(MAX_ITER=100, STEPS=(30, 60), GAMMA=0.5, WARMUP_ITERS=0)
    got = _lrs(cfg, [0, 29, 30, 59, 60, 99])
    want = {0: 1.0, 29: 1.0, 30: 0.5, 59: 0.5, 60: 0.25, 99: 0.25}
    for it, m in want.items():
        assert got[it][0] == pytest.approx(m) and got[it][1] == pytest.approx(0.1 * m), it


def test_multistep_linear_and_constant_warmup_and_steps_past_max_iter():
    cfg = _cfg(MAX_ITER=100, STEPS=(50, 200), GAMMA=0.1, WARMUP_ITERS=10, WARMUP_FACTOR=0.01, WARMUP_METHOD="linear")
    got = _lrs(cfg, [0, 5, 10, 49, 50, 99])
    want = {0: 0.01, 5: 0.01 + (1 - 0.01) * 0.5, 10: 1.0, 49: 1.0, 50: 0.1, 99: 0.1}      # step 200 > MAX_ITER is dropped
    for it, m in want.items():
        assert got[it][0] == pytest.approx(m), it
        assert got[it][1] / got[it][0] == pytest.approx(0.1)                          # the backbone group keeps its ratio
    cfg = _cfg(MAX_ITER=100, STEPS=(50,), WARMUP_ITERS=10, WARMUP_FACTOR=0.25, WARMUP_METHOD="constant")
    got = _lrs(cfg, [0, 9, 10])
    assert [got[i][0] for i in (0, 9, 10)] == pytest.approx([0.25, 0.25, 1.0])


def test_poly_and_cosine():
    cfg = _cfg(LR_SCHEDULER_NAME="WarmupPolyLR", MAX_ITER=100, WARMUP_ITERS=0, POLY_LR_POWER=0.9)
    got = _lrs(cfg, [0, 50, 99])
    for it in (0, 50, 99):
        assert got[it][0] == pytest.approx((1 - it / 100) ** 0.9)
    cfg = _cfg(LR_SCHEDULER_NAME="WarmupPolyLR", MAX_ITER=100, WARMUP_ITERS=0, POLY_LR_POWER=1.0, POLY_LR_CONSTANT_ENDING=0.2)
    got = _lrs(cfg, [10, 85, 99])
    assert [got[i][0] for i in (10, 85, 99)] == pytest.approx([0.9, 0.2, 0.2])
    cfg = _cfg(LR_SCHEDULER_NAME="WarmupPolyLR", MAX_ITER=100, WARMUP_ITERS=10, WARMUP_FACTOR=0.1, POLY_LR_POWER=1.0)
    got = _lrs(cfg, [4])
    assert got[4][0] == pytest.approx((0.1 * 0.6 + 0.4) * 0.96)
    cfg = _cfg(LR_SCHEDULER_NAME="WarmupCosineLR", MAX_ITER=100, WARMUP_ITERS=0)
    got = _lrs(cfg, [0, 25, 50, 100 - 1])
    for it in (0, 25, 50, 99):
        assert got[it][0] == pytest.approx(0.5 * (1 + math.cos(math.pi * it / 100)))
        assert got[it][1] == pytest.approx(0.1 * got[it][0])


def test_scheduler_state_dict_round_trip():
    from s2d_amd.solver import build_lr_scheduler
    cfg = _cfg(MAX_ITER=100, STEPS=(30,), WARMUP_ITERS=5, WARMUP_FACTOR=0.1)
    a = _Opt([1.0, 0.1]); sa = build_lr_scheduler(cfg, a)
    for _ in range(33):
        sa.step()
    b = _Opt([1.0, 0.1]); sb = build_lr_scheduler(cfg, b)
    sb.load_state_dict(json.loads(json.dumps(sa.state_dict())))
    assert [g["lr"] for g in b.param_groups] == [g["lr"] for g in a.param_groups]
    sa.step(); sb.step()
    assert sb.get_last_lr() == sa.get_last_lr()


# ---------------------------------------------------------------------------------------------------------------- config
def test_kd_config_has_every_key_the_driver_reads(monkeypatch):
    from s2d_amd import optim
    cfg = _cfg()
    s = cfg.SOLVER
    for k in ("WEIGHT_DECAY_NORM", "WEIGHT_DECAY_EMBED", "CHECKPOINT_PERIOD", "LR_SCHEDULER_NAME", "GAMMA", "WARMUP_METHOD",
              "POLY_LR_POWER", "POLY_LR_CONSTANT_ENDING", "MAX_ITER", "STEPS", "IMS_PER_BATCH", "BASE_LR", "WARMUP_ITERS",
              "WARMUP_FACTOR"):
        assert hasattr(s, k), k
    assert s.WEIGHT_DECAY_NORM == 0.0 and s.LR_SCHEDULER_NAME == "WarmupMultiStepLR" and s.CHECKPOINT_PERIOD == 5000
    assert cfg.SEED == -1 and cfg.TEST.EVAL_PERIOD == 0 and s.AMP.ENABLED is True and s.IMS_PER_BATCH == 4
    d = cfg.DATALOADER
    assert d.ASPECT_RATIO_GROUPING is True and d.FILTER_EMPTY_ANNOTATIONS is True and d.COPY_PASTE is False
    for k in ("COPY_PASTE_RATE", "COPY_PASTE_RANDOM_NUM", "COPY_PASTE_MIN_RATIO", "COPY_PASTE_MAX_RATIO", "COPY_PASTE_DENSIFY_SPARSE"):
        assert hasattr(d, k), k
    assert cfg.INPUT.DENSE_ANNOTATION_SELECTION is True and cfg.INPUT.DISENTANGLE_DISTILLATION_LOADER is False
    for k in ("EMA_MOMENTUM", "EMA_MOMENTUM_SCHEDULE", "EMA_MOMENTUM_END", "EMA_MOMENTUM_UNTIL_STEP"):
        assert hasattr(cfg.MODEL.MASK_FORMER, k), k
    seen = {}

    class _Stub:
        def __init__(self, groups, lr, clip_norm, ema_params):
            seen.update(groups=groups, lr=lr, clip_norm=clip_norm)

    monkeypatch.setattr(optim, "FullModelGradientClippingAdamW", _Stub)
    net = torch.nn.Sequential(torch.nn.Linear(3, 3), torch.nn.LayerNorm(3))
    optim.build_optimizer(cfg, net)                                         # AttributeError on WEIGHT_DECAY_NORM before
    assert seen["lr"] == 1e-6 and seen["clip_norm"] == 0.01
    assert [g["weight_decay"] for g in seen["groups"]] == [0.05, 0.05, 0.0, 0.0]


def test_existing_defaults_unchanged():
    from s2d_amd.config import DEFAULTS
    assert DEFAULTS["DATALOADER"]["NUM_WORKERS"] == 4 and DEFAULTS["SOLVER"]["ACCUM_ITER"] == 1
    assert DEFAULTS["INPUT"]["MIN_SIZE_TRAIN"] == (800,) and DEFAULTS["OUTPUT_DIR"] == "./output"


# ---------------------------------------------------------------------------------------------------------------- dataset
def _rle(h, w, fill=1):
    return {"size": [h, w], "counts": [0, fill, h * w - fill]}


def _doc():
    vids = [{"id": 7, "height": 4, "width": 6, "length": 3, "file_names": ["a/0.jpg", "a/1.jpg", "a/2.jpg"]},
            {"id": 2, "height": 6, "width": 4, "length": 2, "file_names": ["b/0.jpg", "b/1.jpg"]},
            {"id": 9, "height": 4, "width": 4, "length": 2, "file_names": ["c/0.jpg", "c/1.jpg"]}]
    anns = [
        {"id": 1, "video_id": 7, "category_id": 40, "iscrowd": 0, "bboxes": [[0, 0, 1, 1], None, [0, 0, 1, 1]],
         "segmentations": [_rle(4, 6), _rle(4, 6), None]},                                  # frame 1: null bbox, frame 2: null mask
        {"id": 2, "video_id": 7, "category_id": 10, "iscrowd": 1, "bboxes": [[0, 0, 1, 1]] * 3,
         "segmentations": [_rle(4, 6)] * 3},
        {"id": 3, "video_id": 2, "category_id": 10, "bboxes": [[0, 0, 1, 1]] * 2,
         "segmentations": [{"size": [6, 4], "counts": "32"}, _rle(6, 4)]},
        {"id": 4, "video_id": 9, "category_id": 40, "iscrowd": 1, "bboxes": [[0, 0, 1, 1]] * 2,       # all-crowd video
         "segmentations": [_rle(4, 4)] * 2},
    ]
    return {"videos": vids, "annotations": anns, "categories": [{"id": 40, "name": "b"}, {"id": 10, "name": "a"}]}


def test_load_ytvis_train():
    from s2d_amd.data.train_loader import load_ytvis_train
    recs = load_ytvis_train(_doc(), "/r")
    assert [r["video_id"] for r in recs] == [2, 7]                           # sorted by id, the all-crowd video dropped
    v7 = recs[1]
    assert v7["file_names"][0] == os.path.join("/r", "a/0.jpg") and (v7["height"], v7["width"], v7["length"]) == (4, 6, 3)
    assert [[o["id"] for o in fr] for fr in v7["annotations"]] == [[1, 2], [2], [2]]
    assert v7["annotations"][0][0]["category_id"] == 1 and v7["annotations"][0][1]["category_id"] == 0      # 10 -> 0, 40 -> 1
    assert v7["annotations"][0][1]["iscrowd"] == 1 and "iscrowd" not in recs[0]["annotations"][0][0]
    assert [r["video_id"] for r in load_ytvis_train(_doc(), "/r", filter_empty=False)] == [2, 7, 9]


def test_load_ytvis_train_rejects_polygons_and_size_mismatch():
    from s2d_amd.data.train_loader import load_ytvis_train
    d = _doc()
    d["annotations"][0]["segmentations"][0] = [[0, 0, 1, 0, 1, 1]]
    with pytest.raises(NotImplementedError, match="video 7"):
        load_ytvis_train(d, "/r")
    d = _doc()
    d["annotations"][2]["segmentations"][1] = _rle(4, 6)
    with pytest.raises(ValueError, match="video 2"):
        load_ytvis_train(d, "/r")


# ---------------------------------------------------------------------------------------------------------------- sampler
def _records(n=11):
    return [{"width": 6 if i % 3 else 4, "height": 4, "video_id": i} for i in range(n)]


def _take(it, k):
    return [next(it) for _ in range(k)]


def test_sampler_ranks_are_disjoint_and_cover_each_permutation():
    from s2d_amd.data.train_loader import batch_plan, global_indices
    recs = _records(12)
    g = _take(global_indices(12, 5), 36)
    for e in range(3):
        assert sorted(i for _, i in g[12 * e:12 * e + 12]) == list(range(12))
    r0 = [x for b in _take(batch_plan(recs, 5, 2, 0, 2, False), 9) for x in b]
    r1 = [x for b in _take(batch_plan(recs, 5, 2, 1, 2, False), 9) for x in b]
    assert {p for p, _ in r0}.isdisjoint({p for p, _ in r1})
    assert sorted(r0 + r1) == g
    assert [p % 2 for p, _ in r0] == [0] * 18


def test_aspect_buckets():
    from s2d_amd.data.train_loader import batch_plan
    recs = _records(11)
    for b in _take(batch_plan(recs, 3, 3, 0, 1, True), 20):
        assert len(b) == 3 and len({recs[i]["width"] > recs[i]["height"] for _, i in b}) == 1
        assert [p for p, _ in b] == sorted(p for p, _ in b)


def _settings():
    from s2d_amd.config import load_config
    from s2d_amd.data.train_loader import ClipSettings
    return ClipSettings(load_config(KD_CFG, ["INPUT.MIN_SIZE_TRAIN", "(64, 96)"]))


def _synthetic_records(n=6):
    rng = np.random.default_rng(0)
    recs = []
    for v in range(n):
        L, H, W = 8 + v, 60 + 10 * (v % 2), 90 - 20 * (v % 3 == 0)
        annos = [[{"id": 10 * v + k, "category_id": k % 2, "segmentation": _rle(H, W)} for k in range(3) if rng.random() < 0.7]
                 for _ in range(L)]
        recs.append({"file_names": [f"{v}/{t}.jpg" for t in range(L)], "height": H, "width": W, "length": L, "video_id": v,
                     "annotations": annos})
    return recs


def _plan_key(plans):
    return [(p["record"]["video_id"], p["selected"], p["params"].tobytes(), p["out_hw"], p["plane_of"].tolist(), p["gt_ids"].tolist())
            for p in plans]


def test_resumed_loader_plans_equal_the_uninterrupted_ones():
    from s2d_amd.data.train_loader import YTVISTrainLoader
    recs, st = _synthetic_records(), _settings()
    for rank in (0, 1):
        full = YTVISTrainLoader(recs, st, 2, seed=11, rank=rank, world=2, device="cpu").plans()
        first = [_plan_key(next(full)) for _ in range(9)]
        k = 5
        resumed = YTVISTrainLoader(recs, st, 2, seed=11, rank=rank, world=2, start_iter=k, device="cpu").plans()
        assert [_plan_key(next(resumed)) for _ in range(4)] == first[k:k + 4]
    # the global generators are not touched
    random.seed(3); np.random.seed(3)
    a = (random.random(), np.random.rand())
    random.seed(3); np.random.seed(3)
    next(YTVISTrainLoader(recs, st, 2, seed=11, device="cpu").plans())
    assert (random.random(), np.random.rand()) == a


def _cases():
    """the annotation skeletons behind tests/golden/sampling.json (restates make_golden._sampling_cases)"""
    rng = np.random.default_rng(17)
    cases = []
    for L in (12, 30, 7, 3):
        annos = []
        for t in range(L):
            present = [i for i in range(4) if rng.random() < (0.75 if L != 7 else 0.3)]
            annos.append([{"id": i} for i in present])
        cases.append((L, annos))
    return cases


def test_sampling_with_generators_reproduces_the_golden():
    from s2d_amd.data.sampling import dense_frame_selection, random_frame_selection
    g = json.load(open(os.path.join(HERE, "golden", "sampling.json")))
    cases = _cases()
    for e in g["dense"]:
        L, annos = cases[e["case"]]
        sel = dense_frame_selection(annos, L, e["n"], e["range"], e["shuffle"], random.Random(e["seed"]), np.random.RandomState(e["seed"]))
        assert [int(v) for v in sel] == e["sel"], e
    for e in g["random"]:
        sel = random_frame_selection(e["L"], e["n"], e["range"], e["shuffle"], random.Random(e["seed"]), np.random.RandomState(e["seed"]))
        assert [int(v) for v in sel] == e["sel"], e


# ---------------------------------------------------------------------------------------------------------------- driver
def test_checkpoint_schedule_and_last_checkpoint(tmp_path):
    from s2d_amd.train import checkpoints_at, load_resume, save_checkpoint
    saved = {it: checkpoints_at(it, 3, 8) for it in range(8)}
    assert saved == {0: [], 1: [], 2: ["model_0000002.pth"], 3: [], 4: [], 5: ["model_0000005.pth"], 6: [], 7: ["model_final.pth"]}
    assert checkpoints_at(5, 3, 6) == ["model_0000005.pth", "model_final.pth"]
    assert load_resume(str(tmp_path)) is None

    class _S:
        def state_dict(self):
            return {"last_epoch": 3, "base_lrs": [1.0]}
    net = torch.nn.Linear(2, 2)
    save_checkpoint(str(tmp_path), "model_0000002.pth", net, _S(), _S(), 2, seed=1234)
    assert (tmp_path / "last_checkpoint").read_text() == "model_0000002.pth"
    ck = load_resume(str(tmp_path))
    assert set(ck) == {"model", "optimizer", "scheduler", "iteration", "seed"} and ck["iteration"] == 2 and ck["seed"] == 1234
    assert torch.equal(ck["model"]["weight"], net.weight.detach())


def test_ema_momentum_schedule_of_the_driver():
    from s2d_amd.optim import ema_momentum_schedule
    from s2d_amd.train import ema_momentum_at
    cfg = _cfg()
    assert ema_momentum_at(cfg, 0) == ema_momentum_at(cfg, 17) == cfg.MODEL.MASK_FORMER.EMA_MOMENTUM
    from s2d_amd.config import load_config
    cfg = load_config(KD_CFG, ["MODEL.MASK_FORMER.EMA_MOMENTUM_SCHEDULE", "True", "MODEL.MASK_FORMER.EMA_MOMENTUM", "0.9",
                               "MODEL.MASK_FORMER.EMA_MOMENTUM_END", "0.99", "MODEL.MASK_FORMER.EMA_MOMENTUM_UNTIL_STEP", "100"])
    assert ema_momentum_at(cfg, 0) == 0.9
    assert ema_momentum_at(cfg, 1) == pytest.approx(ema_momentum_schedule(0, 0.9, 0.99, 100)) == pytest.approx(0.9)
    assert ema_momentum_at(cfg, 51) == pytest.approx(ema_momentum_schedule(50, 0.9, 0.99, 100))


@pytest.mark.parametrize("opts,match", [(["INPUT.DISENTANGLE_DISTILLATION_LOADER", "True"], "DISENTANGLE"),
                                        (["SOLVER.OPTIMIZER", "SGD"], "OPTIMIZER")])
def test_cli_rejections(tmp_path, opts, match):
    from s2d_amd.train import main
    with pytest.raises(ValueError, match=match):
        main(["--config-file", KD_CFG, "--train-json", str(tmp_path / "x.json"), "--image-root", str(tmp_path), "--output-dir",
              str(tmp_path / "out")] + opts)


def test_cli_rejects_indivisible_batch(monkeypatch):
    from s2d_amd.train import check_config
    with pytest.raises(ValueError, match="divisible"):
        check_config(_cfg(IMS_PER_BATCH=3), world=2)


# ---------------------------------------------------------------------------------------------------------------- collectives
class _StubDist:
    """a process group of two ranks with the given backend string that records where each collective's tensor lives"""

    class ReduceOp:
        SUM = "sum"

    def __init__(self, backend):
        self.backend, self.seen = backend, []

    def is_initialized(self):
        return True

    def get_world_size(self):
        return 2

    def get_backend(self):
        return self.backend

    def all_reduce(self, t, op=None):
        self.seen.append(("all_reduce", t.device.type))
        t.mul_(2)                                                        # both ranks hold the same values

    def broadcast(self, t, src):
        self.seen.append(("broadcast", t.device.type))


def test_driver_collectives_run_where_the_backend_can_run_them():
    from s2d_amd.train import _reduce_losses, _shared_seed, collective_device
    cuda = torch.device("cuda", 3)
    assert collective_device(_StubDist("nccl"), cuda) == cuda                   # an nccl group has no CPU backend
    assert collective_device(_StubDist("cpu:gloo,cuda:nccl"), cuda) == cuda
    assert collective_device(_StubDist("gloo"), cuda) == torch.device("cpu")
    g = _StubDist("gloo")
    assert _reduce_losses([1.5, 2.0], g, cuda) == [1.5, 2.0]
    assert _shared_seed(-1, g, cuda) >= 0 and _shared_seed(7, g, cuda) == 7
    assert g.seen == [("all_reduce", "cpu"), ("broadcast", "cpu")]
    n = _StubDist("nccl")                                                 # the device the driver passes is where they go
    assert _reduce_losses([1.5, 2.0], n, torch.device("cpu")) == [1.5, 2.0]
    assert n.seen == [("all_reduce", "cpu")]
