"""The routing function of the dense dispatcher (csrc/gemm_route.h) on a CPU: which kernel family and template instantiation a launch of
s2d_launch_gemm_bf16x3 takes, read through the test hook s2d_gemm_route_describe (no HIP call, no GPU) and compared with
tests/golden/gemm_routes.json -- the answers of the dispatcher as it was before the decision became one function (every launch of
that dispatcher replaced by its route name and run as a host program; profiles/gemm_route/parity.txt has the full comparison)."""
import ctypes
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAMILIES = ("rows", "small_m", "f16_ws", "f16_hi", "f16", "conv3x3_halo", "conv7x7s2_stem", "w128", "t<2", "t<4", "err_arg")
# GemmSwitches' members in order, with their defaults (csrc/gemm_route.h)
SWITCH_DEFAULTS = (("rows", 1), ("small", 1), ("ws", 0), ("hi", 2), ("hi_pre", 1), ("pipe", 1), ("w128", 1), ("wm", 0), ("halo", 1), ("halo64", 1),
                   ("halo_pipe", 0), ("stem", 1), ("stem_ph", 8))


@pytest.fixture(scope="module")
def describe():
    from s2d_amd.build import build
    dll = ctypes.CDLL(build(verbose=False))
    fn = dll.s2d_gemm_route_describe
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.POINTER(ctypes.c_long), ctypes.c_int, ctypes.POINTER(ctypes.c_int), ctypes.c_char_p, ctypes.c_int]

    def call(launch, flags, switches, out_len=128):
        sw = [d if s is None else s for s, (_, d) in zip(switches, SWITCH_DEFAULTS)]
        buf = ctypes.create_string_buffer(out_len)
        n = fn((ctypes.c_long * len(launch))(*launch), flags, (ctypes.c_int * len(sw))(*sw), buf, out_len)
        return n, buf.value.decode()
    return call


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(ROOT, "tests", "golden", "gemm_routes.json")) as f:
        return json.load(f)["cases"]


def _family(route):
    return next(f for f in FAMILIES if route == f or route.startswith(f + "<") or (f.startswith("t<") and route.startswith(f + ",")))


def test_golden_table_covers_every_family_and_switch(golden):
    """a shrunken table cannot pass: every route family, and every switch at a non-default value, occurs"""
    assert len(golden) >= 300
    assert {_family(c["route"]) for c in golden} == set(FAMILIES)
    assert all(len(c["launch"]) == 21 and len(c["switches"]) == len(SWITCH_DEFAULTS) for c in golden)
    for i, (name, dflt) in enumerate(SWITCH_DEFAULTS):
        assert any(c["switches"][i] not in (None, dflt) for c in golden), name
    # the values the GPU tests force (test_gpu_dense.py, test_gpu_gemm_rows.py, test_gpu_forward_c4.py)
    for name, value in (("ws", 2), ("w128", 2), ("halo", 2), ("halo_pipe", 0), ("halo_pipe", 1), ("rows", 0), ("rows", 2)):
        i = [n for n, _ in SWITCH_DEFAULTS].index(name)
        assert any(c["switches"][i] == value for c in golden), (name, value)


def test_routes_equal_the_previous_dispatcher(describe, golden):
    bad = []
    for c in golden:
        n, got = describe(c["launch"], c["flags"], c["switches"])
        if got != c["route"] or n != len(got):
            bad.append((c["why"], c["launch"], c["flags"], c["switches"], c["route"], got))
    assert not bad, f"{len(bad)} of {len(golden)} routes differ, first: {bad[:3]}"


def test_describe_reports_a_short_buffer(describe):
    n, got = describe([942080, 256, 256, 256, 256, 256, 256, 256, 0, 0, 256, 1] + [0] * 9, 2 | 4 | 256, [None] * 13, out_len=4)
    assert n < 0
    assert describe([942080, 256, 256, 256, 256, 256, 256, 256, 0, 0, 256, 1] + [0] * 9, 2 | 4 | 256, [None] * 13) == (4, "rows")


def test_one_reader_for_the_kernel_switches():
    """every kernel switch of csrc/ is read through s2d_env_int (common.h): getenv appears there and nowhere else"""
    csrc = os.path.join(ROOT, "s2d_amd", "csrc")
    hits = []
    for f in sorted(os.listdir(csrc)):
        if f.endswith((".hip", ".h")):
            with open(os.path.join(csrc, f)) as src:
                hits += [(f, i + 1) for i, line in enumerate(src) if "getenv" in line]
    assert len(hits) == 1 and hits[0][0] == "common.h", hits
