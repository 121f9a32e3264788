"""Windowed inference, the parts that need no GPU: the window plan, the config keys and their refusal, the declared entry points
(tests/test_abi_cpu.py checks that the built library exports every declared symbol)."""
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIG = os.path.join(ROOT, "tests", "golden", "kd_config.json")
TEST_KEYS = "MODEL.MASK_FORMER.TEST."


def _owned(plan, O):
    """frames every window writes: window 0 all of its own, window w >= 1 those past the O it shares with w - 1"""
    return [list(range(s if w == 0 else s + O, e)) for w, (s, e) in enumerate(plan)]


@pytest.mark.parametrize("T,W,O,want", [
    (5, 8, 3, [(0, 5)]),                                              # T < W
    (8, 8, 3, [(0, 8)]),                                              # T == W
    (1, 2, 1, [(0, 1)]),
    (18, 8, 3, [(0, 8), (5, 13), (10, 18)]),                          # exact multiple of the stride
    (20, 8, 3, [(0, 8), (5, 13), (10, 18), (15, 20)]),
    (9, 8, 3, [(0, 8), (5, 9)]),                                      # the shortest tail there is: O + 1 frames, one of them owned
    (14, 6, 2, [(0, 6), (4, 10), (8, 14)]),
    (7, 4, 3, [(0, 4), (1, 5), (2, 6), (3, 7)]),                      # O = W - 1: stride 1
    (36, 16, 2, [(0, 16), (14, 30), (28, 36)]),
])
def test_plan_windows_cases(T, W, O, want):
    from s2d_amd.modeling.window_inference import plan_windows
    assert plan_windows(T, W, O) == want


def test_plan_windows_invariants_over_a_grid():
    """every frame owned exactly once; consecutive windows share exactly O frames; no window longer than W or -- the tail that a
    plan by stride alone would leave -- shorter than O + 1 (it would own nothing, and is merged into its predecessor)"""
    from s2d_amd.modeling.window_inference import plan_windows
    for W in range(2, 12):
        for O in range(1, W):
            for T in range(1, 60):
                plan = plan_windows(T, W, O)
                assert plan[0][0] == 0 and plan[-1][1] == T
                if T <= W:
                    assert plan == [(0, T)]
                owned = [f for fs in _owned(plan, O) for f in fs]
                assert owned == list(range(T)), (T, W, O, plan)
                for (s0, e0), (s1, e1) in zip(plan, plan[1:]):
                    assert s1 - s0 == W - O and e0 - s1 == O and e0 - s0 == W, (T, W, O, plan)
                assert all(e - s <= W for s, e in plan)
                assert len(plan) == 1 or plan[-1][1] - plan[-1][0] >= O + 1, (T, W, O, plan)
                assert all(e < T for _, e in plan[:-1])               # the last window is the first whose end reaches T


@pytest.mark.parametrize("T,W,O", [(0, 4, 1), (5, 0, 1), (5, 4, 0), (5, 4, 4), (5, 4, 5), (5, -2, 1)])
def test_plan_windows_refuses_bad_arguments(T, W, O):
    from s2d_amd.modeling.window_inference import plan_windows
    with pytest.raises(ValueError):
        plan_windows(T, W, O)


def test_window_keys_have_their_defaults():
    from s2d_amd.config import DEFAULTS, load_config
    t = DEFAULTS["MODEL"]["MASK_FORMER"]["TEST"]
    assert t["WINDOW_INFERENCE"] is False and t["WINDOW_SIZE"] == 0 and t["WINDOW_OVERLAP"] == 0
    cfg = load_config(CONFIG)                                         # a config that predates the keys: the switch is off
    t = cfg.MODEL.MASK_FORMER.TEST
    assert (t.WINDOW_INFERENCE, t.WINDOW_SIZE, t.WINDOW_OVERLAP) == (False, 0, 0)
    cfg = load_config(CONFIG, [TEST_KEYS + "WINDOW_INFERENCE", "True", TEST_KEYS + "WINDOW_SIZE", "16", TEST_KEYS + "WINDOW_OVERLAP", "2"])
    t = cfg.MODEL.MASK_FORMER.TEST
    assert (t.WINDOW_INFERENCE, t.WINDOW_SIZE, t.WINDOW_OVERLAP) == (True, 16, 2)


def _from_config(meta_arch, on, W, O, extra=()):
    from s2d_amd.config import load_config
    from s2d_amd.modeling.meta_arch import META_ARCH_REGISTRY
    opts = ["MODEL.META_ARCHITECTURE", meta_arch, "MODEL.MASK_FORMER.NUM_OBJECT_QUERIES", "12", "MODEL.MASK_FORMER.DEC_LAYERS", "3",
            TEST_KEYS + "WINDOW_INFERENCE", str(on), TEST_KEYS + "WINDOW_SIZE", str(W), TEST_KEYS + "WINDOW_OVERLAP", str(O)]
    cfg = load_config(CONFIG, opts + list(extra))
    return META_ARCH_REGISTRY.get(meta_arch).from_config(cfg)


@pytest.mark.parametrize("meta_arch", ["KDVideoMaskFormer", "VideoMaskFormer"])
def test_from_config_reads_the_window_keys(meta_arch):
    m = _from_config(meta_arch, True, 6, 2)
    assert (m.window_inference, m.window_size, m.window_overlap) == (True, 6, 2)
    m = _from_config(meta_arch, False, 0, 0)
    assert (m.window_inference, m.window_size, m.window_overlap) == (False, 0, 0)
    m = _from_config(meta_arch, False, -3, 7)                         # switch off: the other two keys are not looked at
    assert m.window_inference is False


@pytest.mark.parametrize("meta_arch", ["KDVideoMaskFormer", "VideoMaskFormer"])
@pytest.mark.parametrize("W,O,what", [(0, 1, "WINDOW_SIZE"), (-4, 1, "WINDOW_SIZE"), (8, 0, "WINDOW_OVERLAP"),
                                      (8, 8, "WINDOW_OVERLAP"), (8, 9, "WINDOW_OVERLAP"), (8, -1, "WINDOW_OVERLAP")])
def test_from_config_refuses_bad_window_keys(meta_arch, W, O, what):
    with pytest.raises(ValueError, match=what):
        _from_config(meta_arch, True, W, O)


def test_from_config_refuses_more_queries_than_the_association_takes():
    with pytest.raises(ValueError, match="NUM_OBJECT_QUERIES"):
        _from_config("KDVideoMaskFormer", True, 8, 2, extra=["MODEL.MASK_FORMER.NUM_OBJECT_QUERIES", "120"])
    _from_config("KDVideoMaskFormer", False, 8, 2, extra=["MODEL.MASK_FORMER.NUM_OBJECT_QUERIES", "120"])


def test_window_entry_points_are_declared():
    import ctypes
    from s2d_amd._lib import parse_header
    protos = parse_header()
    types, ret = protos["s2d_window_pair_counts"]
    assert ret == "int" and len(types) == 9 and types[2] is ctypes.c_long and types[3] is ctypes.c_int
    types, ret = protos["s2d_window_scatter_columns"]
    assert ret == "int" and len(types) == 8 and types[1] is ctypes.c_long and types[6] is ctypes.c_long


def test_window_ops_fail_loudly_without_gpu():
    import torch
    from s2d_amd import ops
    with pytest.raises(RuntimeError):
        ops.window_pair_counts(torch.zeros(64, 12), torch.zeros(64, 12), 9)
