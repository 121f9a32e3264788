"""The host references of tests/matcher_refs.py checked without a GPU: cost64 against the oracle's fp32 restatement of the
reference's formula, the point generator's pinned values, every path case's census against the predicate the case is named for,
and the dominance margin of every planted-assignment case.  This is what makes the GPU cases of tests/test_gpu_matcher_paths.py
mean something."""
import numpy as np
import pytest

from s2d_amd.utils import synth
from tests import matcher_refs as R


def test_cost64_agrees_with_the_fp32_restatement(oracle):
    """moderate case (Q = 37, N = 5, T = 2, 13 x 21 map, 300 points, amplitude-4 logits): the bound of
    test_matcher_cost_vs_oracle_odd_shapes; byte values other than 1 are the same targets"""
    c = R.uniform_case("moderate", 11, 1, 1, 37, 2, 13, 21, 52, 84, [5], 300)
    ref = oracle.matcher_cost(c.cls[0, 0], c.masks[0, 0], c.tgt[0], c.coords[0, 0][None], *R.WEIGHTS)
    got, scale = R.cost64(oracle, c.cls[0, 0], c.masks[0, 0], c.tgt[0], c.coords[0, 0][None], *R.WEIGHTS)
    np.testing.assert_allclose(got, ref, rtol=3e-5, atol=3e-5 * np.abs(ref).max())
    assert scale >= np.abs(got).max() * 0.5
    got255, _ = R.cost64(oracle, c.cls[0, 0], c.masks[0, 0], c.tgt[0] * 255, c.coords[0, 0][None], *R.WEIGHTS)
    assert np.array_equal(got, got255)


# 24-bit numerators (u, v) of points 0..2 of problems 0 and 1 at seed 5
PINNED_SEED5 = [[[3737596, 11726012], [14183639, 4463909], [12138506, 4057869]],
                [[4612038, 8080244], [7608154, 16338379], [9355612, 13018748]]]


def test_matcher_points_pinned():
    a = R.matcher_points(5, 3, 1000)
    assert a.dtype == np.float32 and a.shape == (3, 1000, 2)
    assert (a >= 0).all() and (a < 1).all()
    assert np.array_equal(a * 16777216.0, np.round(a * 16777216.0))          # 24-bit mantissas: exact float32 values
    assert not np.array_equal(a[0], a[1]) and not np.array_equal(a[1], a[2])
    assert not np.array_equal(a, R.matcher_points(6, 3, 1000))
    assert np.array_equal(a[:, :10], R.matcher_points(5, 3, 10))             # point i does not depend on P
    assert abs(float(a.mean()) - 0.5) < 0.02
    # mix64 is splitmix64's finaliser: its first outputs from state 0 are published (0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4)
    with np.errstate(over="ignore"):
        z = R._mix64(np.array([0, 0x9E3779B97F4A7C15], np.uint64))
    assert [int(v) for v in z] == [0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4]
    # first values of seed 5: the array code against the same recurrence in python integers, and against the pinned literals
    pins = (a[:2, :3] * 16777216.0).astype(np.int64)

    def mix(z):
        M = (1 << 64) - 1
        z = (z + 0x9E3779B97F4A7C15) & M
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M
        return z ^ (z >> 31)
    for prob in range(2):
        for i in range(3):
            r = mix(5 ^ mix((prob * 0xD1342543DE82EF95 + i) & ((1 << 64) - 1)))
            assert pins[prob, i].tolist() == [r & 0xFFFFFF, (r >> 32) & 0xFFFFFF]
    assert pins.tolist() == PINNED_SEED5


def test_census_on_hand_built_batches():
    """the census itself on point sets small enough to check by hand (5 x 24 map)"""
    rng = synth.rng_for(1, 1)
    # 32 points in cells 0..21 of row 1: span = (21 + 3) & ~1 = 24 == wm: direct; 32 points in cells 0..19 of row 2: span 22: staged
    cells = R._run(24, 22) + R._run(48, 20)
    pts = R.points_at(rng, R.taps_of_cells(rng, cells, 5, 24), 5, 24)
    cen = R.batch_census(pts[None], 5, 24)
    assert [(b[0], b[1], b[2], b[3]) for b in cen["batches"][0]] == [("D", 24, 24, 32), ("S", 22, 48, 32)]
    assert cen["staged"][0] == 1 and cen["direct"][0] == 1 and cen["partial"][0] == 0 and cen["absent"][0] == 14
    assert cen["row_cross"][0] == 0 and cen["lower_past"][0] == 0 and cen["bottom"][0] == 0
    # 40 points in the last cell: one full and one 8-point batch, lower run past the map, taps at x1 = wm and y1 = hm
    pts = R.points_at(rng, R.taps_of_cells(rng, [119] * 40, 5, 24), 5, 24)
    cen = R.batch_census(pts[None], 5, 24)
    assert [b[3] for b in cen["batches"][0]] == [32, 8] and cen["partial"][0] == 1
    assert cen["right"][0] == 1 and cen["bottom"][0] == 1 and cen["lower_past"][0] == 1 and cen["left"][0] == 0
    # the device sorts stably by clamped cell: taps at -1 sort with column / row 0
    pts = R.points_at(rng, [(-1, -1)] * 16 + [(0, 0)] * 16, 5, 24)
    cen = R.batch_census(pts[None], 5, 24)
    assert cen["batches"][0] == [("S", 2, 0, 32)] and cen["left"][0] == 1 and cen["top"][0] == 1


@pytest.mark.parametrize("name,hm,wm", R.path_case_ids())
def test_path_case_census_satisfies_its_predicate(name, hm, wm):
    for Q in (100, 37):
        c = R.path_case(name, hm, wm, Q)
        assert c.coords.min() >= 0 and c.coords.max() <= 1
        assert R.edge_margin(c.coords, hm, wm) >= 1e-3
        cen = c.census()
        print(f"census {c.name}: P {c.P} " + R.census_line(cen))
        assert c.predicate(cen, 0), R.census_line(cen)
        assert c.T <= 2 and c.NL <= 2


def test_path_cases_between_them_take_every_branch():
    """over all path cases: staged and direct batches, both slack rows, both out-of-map tap rows, a run across a row end, a lower
    run past the map, a partial batch, chunks with no batch, chunks with more than one batch, and spans on both sides of wm and of SPANMAX"""
    seen, spans = set(), set()
    for name, hm, wm in R.path_case_ids():
        cen = R.path_case(name, hm, wm, 37).census()
        for k in ("staged", "direct", "partial", "absent", "left", "right", "top", "bottom", "row_cross", "lower_past"):
            if cen[k][0]:
                seen.add(k)
        if len(cen["batches"][0]) > R.CHM:
            seen.add("two_per_chunk")
        spans |= {(wm, b[1], b[0]) for b in cen["batches"][0]}
    assert seen == {"staged", "direct", "partial", "absent", "left", "right", "top", "bottom", "row_cross", "lower_past", "two_per_chunk"}
    assert {(24, 22, "S"), (24, 24, "D"), (26, 24, "S"), (26, 26, "D"), (25, 24, "S"), (21, 20, "S"), (21, 22, "D")} <= spans


@pytest.mark.parametrize("A", [4, 30, 1000])
@pytest.mark.parametrize("N", [6, 40])
def test_planted_assignment_dominates(oracle, A, N):
    """(g) of the GPU module: every planted entry is its column's minimum by more than 4 x the entry-check bound -- a device matrix
    inside the bound (each entry off by at most 3e-5 scale, so a difference by at most 2 x that) has the same column minima with
    a factor 2 to spare, and distinct column minima are the optimal assignment"""
    c = R.trained_case(A, N)
    C, scale = R.cost64(oracle, c.cls[0, 0], c.masks[0, 0], c.tgt[0], c.coords[0, 0][None], *R.WEIGHTS)
    m = R.dominance(C, scale, N)
    print(f"dominance trained-A{A}-N{N}: smallest margin {m:.1f} x (3e-5 x scale), scale {scale:.4g}, required > 4")
    assert m > 4
    assert np.abs(c.masks).max() <= A and c.T <= 2 and c.NL <= 2
    assert (c.tgt.reshape(N, -1).sum(-1) > 0).all()
