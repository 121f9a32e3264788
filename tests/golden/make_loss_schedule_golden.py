#!/usr/bin/env python3
"""Golden of the loss-weight schedules: the reference's own `linear_weight_update`, `cosine_weight_update` and
`update_loss_weights` (model_training/mask2former_video/engine/train_loop.py) on a grid of inputs.  Container-only; re-run with

    python tests/golden/make_loss_schedule_golden.py

train_loop.py imports detectron2 at module level, which is not installed, so the module is not imported: the three top-level
function nodes are compiled from the file's AST where it lies and executed in a namespace holding `math` and `copy`.  Nothing is
copied.

Output loss_schedule.json: {"update": rows of {fn, weight, step, start, end, min_weight, kd, out}, "dict": rows of {fn, step,
start, end, original, minimum, out}}.  `out` is the double the function returned; JSON round-trips doubles exactly (repr).

Rows: both functions, kd true and false, steps before `start`, at `start`, inside the range, at `end` and past `end`, min_weight
0, 0.1 and 1 times the weight, start 0 and a non-zero start; update_loss_weights on the 36-key dict of DEC_LAYERS 6 (6 base keys and
their `_<i>` aux keys)."""
import ast
import copy
import json
import math
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import _ref_shim as R  # noqa: E402

TRAIN_LOOP = os.path.join(R.MT, "mask2former_video", "engine", "train_loop.py")
NAMES = ("linear_weight_update", "cosine_weight_update", "update_loss_weights")


def reference_functions():
    tree = ast.parse(open(TRAIN_LOOP).read(), TRAIN_LOOP)
    keep = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in NAMES]
    assert sorted(n.name for n in keep) == sorted(NAMES), "the schedule functions were not found in train_loop.py"
    ns = {"math": math, "copy": copy}
    exec(compile(ast.Module(body=keep, type_ignores=[]), TRAIN_LOOP, "exec"), ns)
    return {n: ns[n] for n in NAMES}


def main():
    fns = reference_functions()
    update = []
    for fn in ("linear_weight_update", "cosine_weight_update"):
        for kd in (False, True):
            for weight in (5.0, 2.0, 0.3):
                for frac in (0.0, 0.1, 1.0):
                    for start, end in ((0, 12), (4, 12), (1000, 32000)):
                        span = end - start
                        steps = sorted({0, start - 1, start, start + 1, start + span // 3, start + span // 2, end - 1, end, end + 1,
                                        end + span // 2} - {-1})
                        for step in steps:
                            mw = weight * frac
                            update.append(dict(fn=fn, weight=weight, step=step, start=start, end=end, min_weight=mw, kd=kd,
                                               out=fns[fn](weight, step, start, end, mw, kd)))
    base = {"loss_ce": 2.0, "loss_mask": 5.0, "loss_dice": 5.0, "kd_loss_ce": 0.0, "kd_loss_mask": 5.0, "kd_loss_dice": 3.0}
    original = dict(base)
    for i in range(5):
        original.update({k + f"_{i}": v for k, v in base.items()})
    assert len(original) == 36
    minimum = {k: v * 0.1 if "kd" not in k else v * 0.25 for k, v in original.items()}
    dicts = []
    for fn in ("linear_weight_update", "cosine_weight_update"):
        for start, end in ((0, 12), (4, 12)):
            for step in (0, 3, 4, 7, 11, 12, 15):
                out = fns["update_loss_weights"](fns[fn], original, step, start, end, minimum)
                dicts.append(dict(fn=fn, step=step, start=start, end=end, original=original, minimum=minimum, out=out))
    path = os.path.join(HERE, "loss_schedule.json")
    with open(path, "w") as fh:
        json.dump({"update": update, "dict": dicts}, fh, indent=0)
        fh.write("\n")
    print(path, len(update), "update rows,", len(dicts), "dict rows")


if __name__ == "__main__":
    main()
