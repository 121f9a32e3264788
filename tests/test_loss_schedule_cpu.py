"""CPU checks of the loss-weight schedules (s2d_amd/loss_schedule.py): the restated update functions against the doubles the
reference's functions returned (tests/golden/loss_schedule.json, exact equality), LossWeightSchedule.weights_at against a stateful
simulator that mutates a dict in the reference trainer's statement order, the driver's refusals, the config defaults."""
import copy
import itertools
import json
import logging
import math
import os
import types

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
KD_CFG = os.path.join(HERE, "golden", "kd_config.json")
GOLDEN = os.path.join(HERE, "golden", "loss_schedule.json")
MF = "MODEL.MASK_FORMER."


def schedule_cfg(scheduler="constant", D=0, start=0, end=-1, smin=0.0, kmin=0.0, only_sup=False, only_kd=False, max_iter=12,
                 extra=()):
    from s2d_amd.config import load_config
    return load_config(KD_CFG, [MF + "KD_WEIGHT_SCHEDULER", scheduler, MF + "LOSS_WEIGHT_DECAY_STEP", str(D),
                                MF + "KD_WEIGHT_DECAY_START", str(start), MF + "KD_WEIGHT_DECAY_END", str(end),
                                MF + "SUPERVISED_MIN_WEIGHT", repr(smin), MF + "KD_MIN_WEIGHT", repr(kmin),
                                MF + "DECAY_ONLY_SUPERVISED_LOSS", str(only_sup), MF + "DECAY_ONLY_KD_LOSS", str(only_kd),
                                "SOLVER.MAX_ITER", str(max_iter)] + list(extra))


def weight_dict(dec_layers=6, base=None):
    """the dict KDVideoMaskFormer.from_config builds: 6 base keys and their `_<i>` aux keys"""
    base = base or {"loss_ce": 2.0, "loss_mask": 5.0, "loss_dice": 5.0, "kd_loss_ce": 0.0, "kd_loss_mask": 5.0, "kd_loss_dice": 3.0}
    wd = dict(base)
    for i in range(dec_layers - 1):
        wd.update({k + f"_{i}": v for k, v in base.items()})
    return wd


def simulate(cfg, wd0, n_iter):
    """the weight dict the reference's `self.model(data)` sees at every iteration 0 .. n_iter - 1: one dict mutated in the order
    of CustomAMPTrainer.run_step (train_loop.py:692-699 step decay before the forward, :776-811 scheduler update after it), with
    the trainer's own attribute set-up (:311-359).  Written against the trainer, not against weights_at."""
    from s2d_amd.loss_schedule import cosine_weight_update, linear_weight_update, update_loss_weights
    mf = cfg.MODEL.MASK_FORMER
    crit = types.SimpleNamespace(weight_dict=dict(wd0))
    decay_step = int(mf.LOSS_WEIGHT_DECAY_STEP)
    scheduler, kd_min, sup_min = mf.KD_WEIGHT_SCHEDULER, mf.KD_MIN_WEIGHT, mf.SUPERVISED_MIN_WEIGHT
    start, end = int(mf.KD_WEIGHT_DECAY_START), int(mf.KD_WEIGHT_DECAY_END)
    if end == -1:
        end = cfg.SOLVER.MAX_ITER
    original = copy.deepcopy(crit.weight_dict)
    minimum = {k: v * sup_min if ("kd" not in k) else v * kd_min for k, v in original.items()}
    seen = []
    for it in range(n_iter):
        if it == decay_step and decay_step > 0:
            for k in crit.weight_dict.keys():
                if "kd_" not in k:
                    crit.weight_dict[k] *= sup_min
        seen.append(dict(crit.weight_dict))                                   # loss_dict = self.model(data)
        if scheduler in ["linear", "cosine"]:
            fn = linear_weight_update if scheduler == "linear" else cosine_weight_update
            if mf.DECAY_ONLY_SUPERVISED_LOSS:
                crit.weight_dict.update(update_loss_weights(fn, {k: v for k, v in original.items() if "kd_" not in k}, it, start, end,
                                                            {k: v for k, v in minimum.items() if "kd_" not in k}))
            elif mf.DECAY_ONLY_KD_LOSS:
                crit.weight_dict.update(update_loss_weights(fn, {k: v for k, v in original.items() if "kd_" in k}, it, start, end,
                                                            {k: v for k, v in minimum.items() if "kd_" in k}))
            else:
                crit.weight_dict = update_loss_weights(fn, original, it, start, end, minimum)
    return seen


# ------------------------------------------------------------------------------------------------------------ golden rows
@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as fh:
        return json.load(fh)


def test_update_functions_equal_the_reference_doubles(golden):
    from s2d_amd import loss_schedule as LS
    rows = golden["update"]
    seen = set()
    for r in rows:
        got = getattr(LS, r["fn"])(r["weight"], r["step"], r["start"], r["end"], r["min_weight"], r["kd"])
        assert got == r["out"], r
        s, e = r["start"], r["end"]
        where = "before" if r["step"] < s else "start" if r["step"] == s else "inside" if r["step"] < e else "end" if r["step"] == e else "past"
        seen.add((r["fn"], r["kd"], where, r["min_weight"] == 0.0, r["min_weight"] == r["weight"], s != 0))
    for fn in ("linear_weight_update", "cosine_weight_update"):                # the rows cover what they are meant to
        for kd in (False, True):
            assert {w for f, k, w, *_ in seen if f == fn and k == kd} == {"before", "start", "inside", "end", "past"}
            assert any(z for f, k, _, z, _, _ in seen if f == fn and k == kd) and any(o for f, k, _, _, o, _ in seen if f == fn and k == kd)
            assert any(n for f, k, *_, n in seen if f == fn and k == kd)
    past = [r for r in rows if r["step"] > r["end"] and not r["kd"] and r["min_weight"] == 0.0 and r["fn"] == "linear_weight_update"]
    assert past and all(r["out"] < 0 for r in past)                          # no clamp above 1: the reference extrapolates
    before = [r for r in rows if r["step"] < r["start"]]
    at_start = {(r["fn"], r["weight"], r["start"], r["end"], r["min_weight"], r["kd"]): r["out"] for r in rows if r["step"] == r["start"]}
    assert before and all(r["out"] == at_start[(r["fn"], r["weight"], r["start"], r["end"], r["min_weight"], r["kd"])]
                          for r in before)                                    # q < 0 -> 0: before the start nothing moves


def test_update_loss_weights_equals_the_reference_on_36_keys(golden):
    from s2d_amd import loss_schedule as LS
    assert golden["dict"]
    for r in golden["dict"]:
        assert len(r["original"]) == 36
        orig = dict(r["original"])
        got = LS.update_loss_weights(getattr(LS, r["fn"]), orig, r["step"], r["start"], r["end"], r["minimum"])
        assert got == r["out"] and list(got) == list(r["out"]), (r["fn"], r["step"])
        assert orig == r["original"] and got is not orig


# ------------------------------------------------------------------------------------------------------------ weights_at
GRID = list(itertools.product(("constant", "linear", "cosine"), ((False, False), (True, False), (False, True), (True, True)),
                              (0, 3, 7), (0, 4)))


@pytest.mark.parametrize("scheduler,flags,D,start", GRID)
def test_weights_at_equals_the_stateful_trainer(scheduler, flags, D, start):
    from s2d_amd.loss_schedule import LossWeightSchedule
    cfg = schedule_cfg(scheduler, D, start, -1, 0.1, 0.25, flags[0], flags[1], max_iter=12)
    wd0 = weight_dict()
    want = simulate(cfg, wd0, 12)
    s = LossWeightSchedule(cfg, wd0)
    assert s.W0 == wd0 and s.W0 is not wd0 and s.D == D and s.start == start and s.end == 12
    assert s.active == (D > 0 or scheduler != "constant")
    for i in range(12):
        got = s.weights_at(i)
        assert got == want[i], (i, {k: (got[k], want[i][k]) for k in got if got[k] != want[i][k]})
        assert s.weights_at(i) == got                                         # pure: asking twice, or out of order, changes nothing
    assert s.weights_at(0) == wd0


@pytest.mark.parametrize("scheduler,flags,D", [("linear", (False, False), 3), ("cosine", (True, False), 7), ("linear", (True, True), 7)])
def test_step_decay_under_a_schedule_lasts_one_iteration(scheduler, flags, D):
    """a scheduled supervised key is multiplied at i == D and overwritten by the scheduler for i == D + 1"""
    from s2d_amd.loss_schedule import LossWeightSchedule, cosine_weight_update, linear_weight_update
    cfg = schedule_cfg(scheduler, D, 0, -1, 0.1, 0.25, flags[0], flags[1], max_iter=12)
    wd0 = weight_dict()
    want = simulate(cfg, wd0, 12)
    s = LossWeightSchedule(cfg, wd0)
    fn = linear_weight_update if scheduler == "linear" else cosine_weight_update
    for i, k in itertools.product((D - 1, D, D + 1), ("loss_mask", "loss_dice_2")):
        plain = fn(wd0[k], i - 1, 0, 12, wd0[k] * 0.1, kd=False)
        assert s.weights_at(i)[k] == want[i][k] == (plain * 0.1 if i == D else plain)
    assert s.weights_at(D)["kd_loss_mask"] == want[D]["kd_loss_mask"]


def test_unscheduled_supervised_keys_stay_decayed():
    from s2d_amd.loss_schedule import LossWeightSchedule
    cfg = schedule_cfg("linear", 3, 0, -1, 0.1, 0.25, False, True, max_iter=12)          # only the kd keys are scheduled
    s = LossWeightSchedule(cfg, weight_dict())
    assert [s.weights_at(i)["loss_mask"] for i in (2, 3, 4, 11)] == [5.0, 5.0 * 0.1, 5.0 * 0.1, 5.0 * 0.1]
    assert s.weights_at(1)["kd_loss_mask"] == 5.0 * 0.25 and s.weights_at(1)["loss_mask_4"] == 5.0


def test_power_of_two_minima_give_dyadic_weights():
    from s2d_amd.loss_schedule import LossWeightSchedule
    cfg = schedule_cfg("linear", 0, 0, -1, 0.25, 0.25, max_iter=16)
    wd0 = weight_dict(base={"loss_ce": 2.0, "loss_mask": 5.0, "loss_dice": 5.0, "kd_loss_ce": 0.0, "kd_loss_mask": 5.0, "kd_loss_dice": 3.0})
    s = LossWeightSchedule(cfg, wd0)
    for i in range(1, 16):
        for k, v in s.weights_at(i).items():
            q = (i - 1) / 16                                          # a dyadic fraction: every product below is exact
            want = wd0[k] * 0.25 + wd0[k] * 0.75 * (q if "kd" in k else 1 - q)
            assert v == want and (v * 256.0).is_integer(), (i, k, v)


# ------------------------------------------------------------------------------------------------------------ refusals, defaults
@pytest.mark.parametrize("kw,name", [(dict(scheduler="exponential"), "KD_WEIGHT_SCHEDULER"),
                                     (dict(scheduler="linear", start=5, end=5), "KD_WEIGHT_DECAY_END"),
                                     (dict(scheduler="cosine", start=8, end=4), "KD_WEIGHT_DECAY_END"),
                                     (dict(scheduler="linear", start=0, end=8), "KD_WEIGHT_DECAY_END"),
                                     (dict(scheduler="cosine", start=0, end=11), "negative"),
                                     (dict(smin=-0.1), "SUPERVISED_MIN_WEIGHT"),
                                     (dict(kmin=-1.0), "KD_MIN_WEIGHT")])
def test_check_config_refuses_by_name(kw, name):
    from s2d_amd.train import check_config
    with pytest.raises(ValueError, match=name):
        check_config(schedule_cfg(max_iter=12, **kw))


def test_check_config_accepts_what_the_schedule_can_run():
    from s2d_amd.train import check_config
    for kw in (dict(), dict(scheduler="linear"), dict(scheduler="cosine", start=4, end=12), dict(scheduler="linear", end=20),
               dict(D=5, smin=0.1), dict(scheduler="constant", start=5, end=5)):
        check_config(schedule_cfg(max_iter=12, **kw))


def test_defaults_are_inactive_and_exposed(tmp_path):
    from s2d_amd.config import load_config
    from s2d_amd.loss_schedule import LossWeightSchedule
    p = tmp_path / "bare.yaml"
    p.write_text("MODEL:\n  META_ARCHITECTURE: KDVideoMaskFormer\n")
    mf = load_config(str(p)).MODEL.MASK_FORMER
    got = {k: getattr(mf, k) for k in ("LOSS_WEIGHT_DECAY_STEP", "KD_WEIGHT_SCHEDULER", "DECAY_ONLY_SUPERVISED_LOSS", "DECAY_ONLY_KD_LOSS",
                                       "SUPERVISED_MIN_WEIGHT", "KD_MIN_WEIGHT", "KD_WEIGHT_DECAY_START", "KD_WEIGHT_DECAY_END")}
    assert got == {"LOSS_WEIGHT_DECAY_STEP": 0.0, "KD_WEIGHT_SCHEDULER": "constant", "DECAY_ONLY_SUPERVISED_LOSS": False,
                   "DECAY_ONLY_KD_LOSS": False, "SUPERVISED_MIN_WEIGHT": 0.0, "KD_MIN_WEIGHT": 0.0, "KD_WEIGHT_DECAY_START": 0.0,
                   "KD_WEIGHT_DECAY_END": -1.0}
    assert isinstance(mf.LOSS_WEIGHT_DECAY_STEP, float) and isinstance(mf.KD_WEIGHT_DECAY_END, float)
    s = LossWeightSchedule(load_config(str(p)), weight_dict())
    assert s.active is False and s.weights_at(7) == weight_dict() and s.scheduled == frozenset()
    s = LossWeightSchedule(load_config(KD_CFG), weight_dict())               # the shipped KD config: minima set, scheduler constant
    assert s.active is False


def test_other_architectures_are_ignored_with_one_warning(caplog):
    from s2d_amd.loss_schedule import LossWeightSchedule
    from s2d_amd.train import check_config
    cfg = schedule_cfg("linear", 3, 0, 8, 0.1, 0.1, max_iter=12, extra=["MODEL.META_ARCHITECTURE", "VideoMaskFormer"])
    wd0 = {"loss_ce": 2.0, "loss_mask": 5.0, "loss_dice": 5.0}
    with caplog.at_level(logging.WARNING, logger="s2d_amd.loss_schedule"):
        check_config(cfg)                                                     # end < MAX_ITER is nobody's business here
        s = LossWeightSchedule(cfg, wd0)
    assert s.active is False and [s.weights_at(i) for i in (0, 3, 9)] == [wd0] * 3
    assert len([r for r in caplog.records if r.name == "s2d_amd.loss_schedule" and r.levelno == logging.WARNING]) == 1
    caplog.clear()
    with caplog.at_level(logging.WARNING, logger="s2d_amd.loss_schedule"):
        LossWeightSchedule(schedule_cfg(extra=["MODEL.META_ARCHITECTURE", "VideoMaskFormer"]), wd0)
    assert not caplog.records                                                 # default keys: nothing to say


def test_apply_sets_a_fresh_dict_and_the_reference_magnitude():
    from s2d_amd.loss_schedule import LossWeightSchedule, weight_rel
    cfg = schedule_cfg("cosine", 2, 0, -1, 0.25, 0.5, max_iter=5)
    wd0 = weight_dict(base={"loss_ce": 0.0, "loss_mask": 5.0, "loss_dice": -7.0, "kd_loss_ce": 0.0, "kd_loss_mask": 5.0, "kd_loss_dice": 5.0})
    model = types.SimpleNamespace(criterion=types.SimpleNamespace(weight_dict=wd0))
    s = LossWeightSchedule(cfg, wd0)
    seen = []
    for i in range(5):
        got = s.apply(model, i)
        assert got is model.criterion.weight_dict and got is not wd0 and all(got is not d for d in seen)
        assert got == s.weights_at(i) and model.loss_weight_ref == 7.0
        seen.append(got)
    assert wd0 == weight_dict(base={"loss_ce": 0.0, "loss_mask": 5.0, "loss_dice": -7.0, "kd_loss_ce": 0.0, "kd_loss_mask": 5.0,
                                    "kd_loss_dice": 5.0}) and s.W0 == wd0
    # the relative magnitude the backward's root scale follows
    assert weight_rel(wd0, None) == 1.0 and weight_rel(wd0, 0.0) == 1.0 and weight_rel({"a": 0.0}, 5.0) == 1.0
    assert weight_rel({"a": 5.0, "b": 0.0}, 5.0) == 1.0 and weight_rel({"a": 5.0 / 128, "b": 0.0}, 5.0) == 2.0 ** -7
    assert weight_rel({"a": -0.05, "b": 0.01}, 5.0) == 2.0 ** round(math.log2(0.01))
