"""The reference trainer's loss-weight schedules (mask2former_video/engine/train_loop.py): the one-off step decay
MODEL.MASK_FORMER.LOSS_WEIGHT_DECAY_STEP (:692-699) and the per-iteration schedule KD_WEIGHT_SCHEDULER `linear` / `cosine`
(:776-811) that anneals the objective from the sparse ground-truth loss to the dense distillation loss.

`linear_weight_update`, `cosine_weight_update` and `update_loss_weights` restate :159-239 in Python floats, statement by
statement, so their results are the reference's doubles bit for bit (tests/golden/loss_schedule.json).  `LossWeightSchedule`
turns the trainer's stateful updates into a pure function of the iteration: `weights_at(i)` is the dict the reference's
`self.model(data)` sees at `self.iter == i` in an uninterrupted run, so a resumed run recomputes it (the reference restarts
from the initial weights on resume).  No GPU is needed to import this module."""
import copy
import logging
import math

_log = logging.getLogger("s2d_amd.loss_schedule")

SCHEDULERS = ("constant", "linear", "cosine")
KD_ARCHITECTURE = "KDVideoMaskFormer"          # the reference gates both mechanisms on this meta-architecture (:302, :692)
BASE_KEYS = ("loss_ce", "loss_mask", "loss_dice", "kd_loss_ce", "kd_loss_mask", "kd_loss_dice")


def linear_weight_update(weight, step, start_step, end_step, min_weight, kd):
    """:159-179.  A supervised weight falls from `weight` to `min_weight`, a kd weight rises from `min_weight` to `weight`;
    q is clamped below 0 only, so past end_step both extrapolate."""
    total_steps = end_step - start_step
    step = step - start_step
    q = step / total_steps
    weight_range = weight - min_weight
    if q < 0:
        q = 0
    weight_change_factor = (1 - q) if not kd else q
    weight_change = weight_range * weight_change_factor
    new_weight = min_weight + weight_change
    return new_weight


def cosine_weight_update(weight, step, start_step, end_step, min_weight, kd):
    """:181-228, the half-cosine between the same end points"""
    total_steps = end_step - start_step
    step = step - start_step
    q = step / total_steps
    if q < 0:
        q = 0
    cosine_decay_factor = 0.5 * (1 + math.cos(math.pi * q))
    weight_range = weight - min_weight
    if not kd:
        new_weight = weight_range * cosine_decay_factor + min_weight
    else:
        cosine_ramp_up_factor = 1.0 - cosine_decay_factor
        new_weight = weight_range * cosine_ramp_up_factor + min_weight
    return new_weight


def update_loss_weights(update_fn, original_weight_dict, step, start_step, end_step, minimum_weight_dict):
    """:230-239: every key of original_weight_dict through update_fn, kd = "kd" in the key"""
    new_weight_dict = copy.deepcopy(original_weight_dict)
    for k in new_weight_dict.keys():
        new_weight_dict[k] = update_fn(original_weight_dict[k], step, start_step, end_step, minimum_weight_dict[k], kd=("kd" in k))
    return new_weight_dict


def weight_rel(weight_dict, ref):
    """2^round(log2(max |current nonzero weight| / ref)): how far the loss weights have moved from the magnitude `ref` that the
    backward's root scale was chosen at (backward.GRAD_SCALE_LOG2).  1.0 without a reference, with a zero reference or with
    all weights zero."""
    if not ref or not math.isfinite(ref):
        return 1.0
    m = max((abs(v) for v in weight_dict.values() if v != 0.0), default=0.0)
    if not (m > 0 and math.isfinite(m)):
        return 1.0
    return math.ldexp(1.0, round(math.log2(m / abs(ref))))


_UPDATE = {"linear": linear_weight_update, "cosine": cosine_weight_update}


def _keys(cfg):
    mf = cfg.MODEL.MASK_FORMER
    end = int(mf.KD_WEIGHT_DECAY_END)
    return dict(scheduler=mf.KD_WEIGHT_SCHEDULER, start=int(mf.KD_WEIGHT_DECAY_START),
                end=int(cfg.SOLVER.MAX_ITER) if end == -1 else end, D=int(mf.LOSS_WEIGHT_DECAY_STEP),
                supervised_min=mf.SUPERVISED_MIN_WEIGHT, kd_min=mf.KD_MIN_WEIGHT,
                only_supervised=bool(mf.DECAY_ONLY_SUPERVISED_LOSS), only_kd=bool(mf.DECAY_ONLY_KD_LOSS))


def check_schedule_config(cfg):
    """the loss-weight settings the training driver refuses, by key name (train.check_config).  Only a KDVideoMaskFormer
    config is checked: for any other architecture the reference never reads the keys."""
    if cfg.MODEL.META_ARCHITECTURE != KD_ARCHITECTURE:
        return
    s = _keys(cfg)
    if s["scheduler"] not in SCHEDULERS:
        raise ValueError(f"MODEL.MASK_FORMER.KD_WEIGHT_SCHEDULER {s['scheduler']!r} is not one of {', '.join(SCHEDULERS)}")
    if s["supervised_min"] < 0:
        raise ValueError(f"MODEL.MASK_FORMER.SUPERVISED_MIN_WEIGHT ({s['supervised_min']}) must not be negative")
    if s["kd_min"] < 0:
        raise ValueError(f"MODEL.MASK_FORMER.KD_MIN_WEIGHT ({s['kd_min']}) must not be negative")
    if s["scheduler"] in _UPDATE:
        if s["end"] <= s["start"]:
            raise ValueError(f"MODEL.MASK_FORMER.KD_WEIGHT_DECAY_END ({s['end']}) must lie after KD_WEIGHT_DECAY_START "
                             f"({s['start']}): the schedule divides by their difference")
        if s["end"] < int(cfg.SOLVER.MAX_ITER):
            raise ValueError(f"MODEL.MASK_FORMER.KD_WEIGHT_DECAY_END ({s['end']}) lies before SOLVER.MAX_ITER ({cfg.SOLVER.MAX_ITER}): "
                             "past the end the schedule extrapolates, so supervised weights fall below their minimum and can "
                             "turn negative; set it to -1 or to MAX_ITER")


class LossWeightSchedule:
    """cfg + the criterion's initial weight dict -> the weight dict of every iteration.

    W0: a copy of weight_dict, every key (the `_<i>` aux keys included); min[k] = W0[k] * SUPERVISED_MIN_WEIGHT for a key
    without "kd" in its name, W0[k] * KD_MIN_WEIGHT otherwise (:355-359); start, end (-1: SOLVER.MAX_ITER) and D as the
    reference reads them (:311-325).  Under SOLVER.ACCUM_ITER > 1 the iteration counts micro-steps, as self.iter does."""

    def __init__(self, cfg, weight_dict):
        s = _keys(cfg)
        self.scheduler, self.start, self.end, self.D = s["scheduler"], s["start"], s["end"], s["D"]
        self.supervised_min, self.kd_min = s["supervised_min"], s["kd_min"]
        self.W0 = copy.deepcopy(dict(weight_dict))
        self.min = {k: v * self.supervised_min if ("kd" not in k) else v * self.kd_min for k, v in self.W0.items()}
        wanted = self.D > 0 or self.scheduler in _UPDATE
        self.active = wanted and cfg.MODEL.META_ARCHITECTURE == KD_ARCHITECTURE
        if wanted and not self.active:
            _log.warning("MODEL.MASK_FORMER.LOSS_WEIGHT_DECAY_STEP / KD_WEIGHT_SCHEDULER are ignored for META_ARCHITECTURE %s: "
                         "loss weights are scheduled for %s only", cfg.MODEL.META_ARCHITECTURE, KD_ARCHITECTURE)
        # the keys the per-iteration schedule rewrites: DECAY_ONLY_SUPERVISED_LOSS is looked at first (:778), then
        # DECAY_ONLY_KD_LOSS (:789), else the whole dict is replaced (:800-811)
        if not self.active or self.scheduler not in _UPDATE:
            self.scheduled = frozenset()
        elif s["only_supervised"]:
            self.scheduled = frozenset(k for k in self.W0 if "kd" not in k)
        elif s["only_kd"]:
            self.scheduled = frozenset(k for k in self.W0 if "kd" in k)
        else:
            self.scheduled = frozenset(self.W0)

    def weights_at(self, i):
        """the weight dict of iteration i, a pure function of i.  The reference updates the dict at the end of run_step, so
        iteration i uses what iteration i - 1 computed and iteration 0 uses W0.  Step decay (:693-699, supervised keys, before
        the forward): at i == D the value in the dict is multiplied by SUPERVISED_MIN_WEIGHT; afterwards the scheduler
        overwrites its own keys and the others stay decayed."""
        if not self.active:
            return dict(self.W0)
        fn = _UPDATE.get(self.scheduler)
        out = {}
        for k, w0 in self.W0.items():
            kd = "kd" in k
            if k in self.scheduled and i >= 1:
                v = fn(w0, i - 1, self.start, self.end, self.min[k], kd=kd)
            else:
                v = w0
            if not kd and self.D > 0:
                if i == self.D:
                    v *= self.supervised_min
                elif i > self.D and k not in self.scheduled:
                    v = w0 * self.supervised_min
            out[k] = v
        return out

    def apply(self, model, i):
        """model.criterion.weight_dict = weights_at(i), a fresh dict, and model.loss_weight_ref = max |W0|: the magnitude the
        backward's root scale was chosen at (weight_rel).  A trainer that keeps the reference's own statements
        (`loss_dict = model(data)`) calls this before them.  Returns the dict."""
        wd = self.weights_at(i)
        model.criterion.weight_dict = wd
        model.loss_weight_ref = max((abs(v) for v in self.W0.values()), default=0.0)
        return wd

    def describe(self):
        """the driver's start line"""
        return {"loss_weight_scheduler": self.scheduler, "start": self.start, "end": self.end, "D": self.D,
                "supervised_min_weight": self.supervised_min, "kd_min_weight": self.kd_min}
