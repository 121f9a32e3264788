"""LR schedulers of the training driver: `build_lr_scheduler(cfg, optimizer)` is what train_net_video.py:126-131 reaches through
detectron2.projects.deeplab.build_lr_scheduler -- WarmupPolyLR from deeplab, anything else detectron2's own
build_lr_scheduler (WarmupMultiStepLR, WarmupCosineLR: a fvcore ParamScheduler wrapped in WarmupParamScheduler, applied by
LRMultiplier).  Neither detectron2 nor fvcore is in the reference tree: these restate their published semantics, parity unpinned.

    WarmupMultiStepLR  GAMMA ** (number of STEPS <= iter); STEPS beyond MAX_ITER are dropped with a warning
    WarmupCosineLR     0.5 * (1 + cos(pi * iter / MAX_ITER))
    warmup (both)      for iter < WARMUP_ITERS: linear from WARMUP_FACTOR * f(0) to f(WARMUP_ITERS), or constant WARMUP_FACTOR * f(0)
    WarmupPolyLR       warmup(iter) * (1 - iter / MAX_ITER) ** POLY_LR_POWER, where warmup(iter) = WARMUP_FACTOR * (1 - a) + a,
                       a = iter / WARMUP_ITERS (linear) or WARMUP_FACTOR (constant) below WARMUP_ITERS, 1 after; with
                       POLY_LR_CONSTANT_ENDING > 0 and no warmup left, never below that fraction

Every parameter group keeps its own initial lr (so BACKBONE_MULTIPLIER survives): lr_g = initial_lr_g * multiplier(iter).  The
scheduler is stepped once per iteration, after the optimizer step."""
import bisect
import logging
import math

_log = logging.getLogger(__name__)


def _warmup_factor_at_iter(method, it, warmup_iters, warmup_factor):
    """detectron2 solver.lr_scheduler._get_warmup_factor_at_iter"""
    if it >= warmup_iters:
        return 1.0
    if method == "constant":
        return warmup_factor
    if method == "linear":
        alpha = it / warmup_iters
        return warmup_factor * (1 - alpha) + alpha
    raise ValueError(f"Unknown warmup method: {method}")


class LRScheduler:
    """LRMultiplier: lr of group g at iteration i = initial_lr_g * multiplier(i); step() moves to the next iteration"""

    def __init__(self, optimizer, multiplier, max_iter):
        self.optimizer, self.multiplier, self.max_iter = optimizer, multiplier, int(max_iter)
        for g in optimizer.param_groups:
            g.setdefault("initial_lr", g["lr"])
        self.base_lrs = [g["initial_lr"] for g in optimizer.param_groups]
        self.last_epoch = 0
        self._apply()

    def _apply(self):
        m = self.multiplier(self.last_epoch)
        for g, lr in zip(self.optimizer.param_groups, self.base_lrs):
            g["lr"] = lr * m

    def step(self):
        self.last_epoch += 1
        self._apply()

    def get_last_lr(self):
        return [g["lr"] for g in self.optimizer.param_groups]

    def state_dict(self):
        return {"last_epoch": self.last_epoch, "base_lrs": list(self.base_lrs)}

    def load_state_dict(self, sd):
        self.last_epoch = int(sd["last_epoch"])
        self.base_lrs = list(sd["base_lrs"])
        self._apply()


def multistep_multiplier(steps, gamma, max_iter):
    def f(it):
        return gamma ** bisect.bisect_right(steps, it)
    return f


def cosine_multiplier(max_iter, end=0.0):
    def f(it):
        return end + 0.5 * (1.0 - end) * (1.0 + math.cos(math.pi * it / max_iter))
    return f


def with_warmup(f, warmup_factor, warmup_iters, method):
    """fvcore WarmupParamScheduler (rescale_interval off): the warmup interval runs from warmup_factor * f(0) to f(warmup_iters)"""
    start, end = warmup_factor * f(0), f(warmup_iters)

    def g(it):
        if it >= warmup_iters:
            return f(it)
        if method == "constant":
            return start
        if method == "linear":
            return start + (end - start) * (it / warmup_iters)
        raise ValueError(f"Unknown warmup method: {method}")
    return g


def poly_multiplier(max_iter, power, constant_ending, warmup_factor, warmup_iters, method):
    """deeplab WarmupPolyLR.get_lr"""
    def f(it):
        w = _warmup_factor_at_iter(method, it, warmup_iters, warmup_factor)
        p = math.pow(1.0 - it / max_iter, power)
        if constant_ending > 0 and w == 1.0 and p < constant_ending:
            return constant_ending
        return w * p
    return f


def build_lr_scheduler(cfg, optimizer):
    s = cfg.SOLVER
    name, max_iter = s.LR_SCHEDULER_NAME, int(s.MAX_ITER)
    if name == "WarmupPolyLR":
        mult = poly_multiplier(max_iter, s.POLY_LR_POWER, s.POLY_LR_CONSTANT_ENDING, s.WARMUP_FACTOR, s.WARMUP_ITERS, s.WARMUP_METHOD)
        return LRScheduler(optimizer, mult, max_iter)
    if name == "WarmupMultiStepLR":
        steps = [x for x in s.STEPS if x <= max_iter]
        if len(steps) != len(s.STEPS):
            _log.warning("SOLVER.STEPS contains values larger than SOLVER.MAX_ITER. These values will be ignored.")
        f = multistep_multiplier(sorted(steps), s.GAMMA, max_iter)
    elif name == "WarmupCosineLR":
        f = cosine_multiplier(max_iter, getattr(s, "BASE_LR_END", 0.0) / s.BASE_LR if getattr(s, "BASE_LR_END", 0.0) else 0.0)
    else:
        raise ValueError(f"Unknown LR scheduler: {name}")
    warmup_iters = min(int(s.WARMUP_ITERS), max_iter)
    if warmup_iters > 0:
        f = with_warmup(f, s.WARMUP_FACTOR, warmup_iters, s.WARMUP_METHOD)
    return LRScheduler(optimizer, f, max_iter)
