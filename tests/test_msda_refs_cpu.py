"""The references and case generators of tests/msda_refs.py are what they claim (no GPU)."""
import numpy as np
import pytest
import torch

from tests import msda_refs as R


def _t(a, dtype=torch.float64):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype)


def _rel(a, b):
    b = np.asarray(b, np.float64)
    return float(np.abs(np.asarray(a, np.float64) - b).max() / max(np.abs(b).max(), 1e-30))


def _torch64(c, grads=False):
    args = (_t(c["value"]), c["shapes"], _t(c["loc"]), _t(c["attn"]))
    if not grads:
        return R.msda_torch(*args).numpy()
    return tuple(t.numpy() for t in R.msda_torch(*args, _t(c["grad_out"])))


@pytest.mark.parametrize("case", ["random", "lattice", "lattice_h1", "lattice_w1", "offgrid", "segments_corners", "nonfinite"])
def test_reference_forward_equals_float64_grid_sample(case):
    """random samples, lattice samples and border samples (and, with grid_sample's undefined coordinates moved outside, the skipped ones)"""
    c = {"random": lambda: R.geometry_case(8, 32, 4, 4, 33), "lattice": lambda: R.lattice_case("pow2"), "lattice_h1": lambda: R.lattice_case("h1", P=6),
         "lattice_w1": lambda: R.lattice_case("w1"), "offgrid": lambda: R.offgrid_case(Lq=24), "segments_corners": lambda: R.segments_case("corners"),
         "nonfinite": R.nonfinite_case}[case]()
    out = R.msda_ref(c["value"], c["shapes"], c["loc"], c["attn"])
    ref = _torch64(c)
    assert np.isfinite(out).all()
    assert _rel(out, ref) < 1e-13


@pytest.mark.parametrize("geom", [(8, 32, 4, 4, 33), (3, 32, 2, 3, 5), (8, 10, 3, 4, 5)])
def test_reference_gradients_equal_float64_autograd_away_from_the_lattice(geom):
    c = R.geometry_case(*geom)
    _, _, _, h_im, w_im = R.cells(c["loc"], c["shapes"])
    assert (np.abs(h_im - np.round(h_im)) > 1e-6).all() and (np.abs(w_im - np.round(w_im)) > 1e-6).all()
    got = R.msda_ref(c["value"], c["shapes"], c["loc"], c["attn"], c["grad_out"])
    ref = _torch64(c, grads=True)
    for g, r, name in zip(got, ref, ("out", "grad_value", "grad_loc", "grad_attn")):
        assert _rel(g, r) < 1e-12, name


@pytest.mark.parametrize("pyr,P", [("pow2", 4), ("h1", 6), ("w1", 4)])
def test_reference_location_gradient_is_the_one_sided_difference_from_the_right_and_below(pyr, P):
    """A sample's share of sum(out * grad_out) is attn * grad_attn(loc), piecewise bilinear in its position, so a forward difference
    over 2^-30 px inside the cell to the right / below is its one-sided derivative.  Every lattice and border sample is compared but
    the ones at exactly -1 in an axis: there the range test (strict, cuh:293) skips the sample -- gradient exactly 0, asserted --
    although the function rises from 0 to its right."""
    c = R.lattice_case(pyr, P=P)
    v, sh, loc, a, go = c["value"], c["shapes"], c["loc"].astype(np.float64), c["attn"].astype(np.float64), c["grad_out"]
    _, _, gl, ga = R.msda_ref(v, sh, loc, a, go)
    tgt = c["props"]["targets"]
    eps = 2.0 ** -30
    norm = np.array([[w, h] for h, w in sh], np.float64)[None, None, None, :, None, :]
    at_minus_one = (tgt == -1).any(-1)
    assert at_minus_one.any() and (gl[at_minus_one] == 0).all() and (ga[at_minus_one] == 0).all()
    for ax in (0, 1):
        step = np.zeros(2)
        step[ax] = eps
        _, _, _, ga2 = R.msda_ref(v, sh, loc + step / norm, a, go)
        fd = a * (ga2 - ga) / eps * norm[..., ax]                     # d/d(loc) = d/d(px) * (W, H)
        keep = ~at_minus_one
        assert keep.mean() > 0.7
        err = np.abs(fd - gl[..., ax])[keep].max() / np.abs(gl[..., ax]).max()
        assert err < 1e-5, (ax, err)


@pytest.mark.parametrize("pyr,P", [("pow2", 4), ("pow2", 6), ("h1", 4), ("h1", 6), ("w1", 4), ("w1", 6)])
def test_lattice_case_is_exact_in_float32_in_any_order(pyr, P):
    """what licenses equality on the GPU: the float64 results are float32 numbers, and a float32 evaluation with every sum reversed gives
    the same bits"""
    c = R.lattice_case(pyr, P=P)
    ref = R.msda_ref(c["value"], c["shapes"], c["loc"], c["attn"], c["grad_out"])
    rev = R.msda_ref(c["value"], c["shapes"], c["loc"], c["attn"], c["grad_out"], dtype=np.float32, reverse=True)
    fwd = R.msda_ref(c["value"], c["shapes"], c["loc"], c["attn"], c["grad_out"], dtype=np.float32)
    for r64, r32, f32, name in zip(ref, rev, fwd, ("out", "grad_value", "grad_loc", "grad_attn")):
        assert np.array_equal(r64.astype(np.float32).astype(np.float64), r64), name
        assert r32.dtype == np.float32 and np.array_equal(r32, r64.astype(np.float32)), name
        assert np.array_equal(f32, r64.astype(np.float32)), name
        assert np.abs(r64).max() > 0
    # the float32 position arithmetic is exact too: same cells, same fractions
    i64, h64, w64, y64, x64 = R.cells(c["loc"], c["shapes"])
    i32, h32, w32, y32, x32 = R.cells(c["loc"], c["shapes"], np.float32)
    assert np.array_equal(i64, i32) and np.array_equal(h64, h32) and np.array_equal(w64, w32)
    assert np.array_equal(y32.astype(np.float64), y64) and np.array_equal(x32.astype(np.float64), x64)
    # the case covers what it is named for, per level and axis: -1.5, -1, -0.5, 0, ..., W - 0.5, W and the floats next to -1 and W
    tgt = c["props"]["targets"]
    near = c["props"]["near_head"]
    for l, (H, W) in enumerate(c["shapes"]):
        for ax, E in ((0, W), (1, H)):
            seen = set(np.unique(tgt[:, :, :near, l, :, ax]).tolist())
            assert set(R.axis_targets(E).tolist()) <= seen
            assert {-1.5, -1.0, -0.5, 0.0, E - 1.0, E - 0.5, float(E)} <= seen
            nb = R.border_neighbours(E)
            assert nb[0] < -1 < nb[1] < -1 + 1e-6 and nb[2] < E < nb[3] and E - nb[2] < 1e-5 * E + 1e-6
            assert set(nb) <= set(np.unique(tgt[:, :, near, l, :, ax]).tolist())
        pairs = {(y, x) for x, y in tgt[:, :, :near, l].reshape(-1, 2).tolist()}
        assert len(pairs) == c["props"]["covered"][l] == len(R.axis_targets(H)) * len(R.axis_targets(W))
    # near-border samples: inside on one side of the border, outside on the other
    assert i64[:, :, near].any() and (~i64[:, :, near]).any()


@pytest.mark.parametrize("pyr", ["pow2", "h1", "w1"])
def test_fused_lattice_case_selects_the_float64_cells_in_float32(pyr):
    c = R.fused_lattice_case(pyr)
    i64, h64, w64, y64, x64 = R.cells_fused(c["oa"], c["shapes"], c["M"], c["P"], np.float64)
    i32, h32, w32, y32, x32 = R.cells_fused(c["oa"], c["shapes"], c["M"], c["P"], np.float32)
    assert np.array_equal(i64, i32) and np.array_equal(h64, h32) and np.array_equal(w64, w32)
    tgt = c["props"]["targets"]
    assert np.array_equal(x64, tgt[..., 0]) and np.array_equal(y64, tgt[..., 1]) and np.array_equal(x32.astype(np.float64), x64)
    for l, (H, W) in enumerate(c["shapes"]):
        assert set(R.axis_targets(W).tolist()) <= set(np.unique(tgt[:, :, :, l, :, 0]).tolist())
        assert set(R.axis_targets(H).tolist()) <= set(np.unique(tgt[:, :, :, l, :, 1]).tolist())
    out, gv, doa = R.fused_ref(c["value"], c["shapes"], c["oa"], c["M"], c["P"], c["grad_out"])
    assert np.isfinite(out).all() and np.isfinite(gv).all() and np.isfinite(doa).all() and np.abs(doa).max() > 0


def test_offgrid_case_reports_the_share_of_float32_cells_that_differ(capsys):
    c = R.offgrid_case()
    diff, free, delib = R.offgrid_disagreement(c)
    with capsys.disabled():
        print(f"\noffgrid: float32 cell != float64 cell on {free:.2e} of the free samples, {delib:.3f} of the deliberate lattice samples "
              f"({int(diff.sum())} of {diff.size})")
    assert free <= 1e-3
    assert delib > 0.01, "non-power-of-two levels should put some lattice samples an ulp across"
    # the fused gradient's restatement of the same thing: one-sided values of the two adjacent cells exist for every deliberate sample
    (hh, wh), (hl, wl) = R.adjacent_cells(c["props"]["targets"])
    i64, h64, w64, _, _ = R.cells(c["loc"], c["shapes"])
    d = c["props"]["deliberate"]
    i32, h32, w32, _, _ = R.cells(c["loc"], c["shapes"], np.float32)
    ok32 = ((h32 == hh) | (h32 == hl)) & ((w32 == wh) | (w32 == wl))
    assert ok32[d & i32].all(), "a deliberate sample's float32 cell is one of the two adjacent to its lattice point"


def test_fused_offgrid_case_lands_beside_its_targets(capsys):
    c = R.fused_lattice_case("offgrid", N=1)
    diff = R.fused_offgrid_disagreement(c)
    with capsys.disabled():
        print(f"\nfused offgrid: float32 cell != float64 cell on {diff.mean():.3f} of the samples (all deliberate lattice / border targets)")
    assert 0.01 < diff.mean() < 0.5
    tgt = c["props"]["targets"]
    (hh, wh), (hl, wl) = R.adjacent_cells(tgt)
    for dt in (np.float64, np.float32):
        ins, h0, w0, y, x = R.cells_fused(c["oa"], c["shapes"], c["M"], c["P"], dt)
        assert np.abs(x - tgt[..., 0]).max() < 1e-4 and np.abs(y - tgt[..., 1]).max() < 1e-4
        assert (((h0 == hh) | (h0 == hl)) & ((w0 == wh) | (w0 == wl)))[ins].all()


def test_segments_case_has_the_stated_per_cell_counts():
    c = R.segments_case("counts")
    got = R.cell_counts(c["loc"], c["shapes"], 0, 0, 0)
    want = {k: v for k, v in R.SEGMENT_COUNTS.items() if v}
    assert got == want and (3, 3) not in got
    assert sorted(R.SEGMENT_COUNTS.values()) == [0, 1, 7, 8, 9, 16, 17]
    assert len(R.cell_counts(c["loc"], c["shapes"], 1, 3, 0)) > 10                 # other (frame, head)s are ordinary
    one = R.segments_case("one_cell")
    ins, h0, w0, _, _ = R.cells(one["loc"], one["shapes"], np.float32)
    assert ins.all() and (h0 == 1).all() and (w0 == 1).all()
    out = R.segments_case("all_outside")
    assert not R.cells(out["loc"], out["shapes"], np.float32)[0].any() and not R.cells(out["loc"], out["shapes"])[0].any()
    cor = R.segments_case("corners")
    ins, h0, w0, _, _ = R.cells(cor["loc"], cor["shapes"], np.float32)
    assert ins.all()
    for l, (H, W) in enumerate(cor["shapes"]):
        cellset = set(zip(h0[:, :, :, l].reshape(-1).tolist(), w0[:, :, :, l].reshape(-1).tolist()))
        assert cellset == {(-1, -1), (H - 1, W - 1)}


@pytest.mark.parametrize("fused", [False, True])
def test_nonfinite_case_rows(fused):
    c = R.fused_nonfinite_case() if fused else R.nonfinite_case()
    bad = c["props"]["bad"]
    if fused:
        N, S = c["oa"].shape[:2]
        M, P, L = c["M"], c["P"], len(c["shapes"])
        raw = c["oa"][..., :M * L * P * 2].reshape(N, S, M, L, P, 2)
        inside = R.cells_fused(c["oa"], c["shapes"], M, P, np.float64)[0]
        out, gv, doa = R.fused_ref(c["value"], c["shapes"], c["oa"], M, P, c["grad_out"])
        D = c["value"].shape[-1] // M
        gl = doa[..., :M * L * P * 2].reshape(N, S, M, L, P, 2)
    else:
        raw = c["loc"]
        M, D = c["value"].shape[2:]
        inside = R.cells(c["loc"], c["shapes"])[0]
        out, gv, gl, ga = R.msda_ref(c["value"], c["shapes"], c["loc"], c["attn"], c["grad_out"])
        assert (ga[bad] == 0).all()
    seen = raw[bad]
    for b in R.BAD:
        assert (np.isnan(seen).any() if np.isnan(b) else (seen == np.float32(b)).any()), b
    assert np.floor(3e9) > 2 ** 31 and not inside[bad].any() and inside[~bad].mean() > (0.5 if fused else 0.999)
    assert np.isfinite(out).all() and np.isfinite(gv).all() and np.isfinite(gl).all()
    assert (gl[bad] == 0).all()
    for n, q, m in c["props"]["all_rows"]:
        assert bad[n, q, m].all() and (out[n, q, m * D:(m + 1) * D] == 0).all()
    assert len(c["props"]["mixed_rows"]) == (42 if fused else 21) and len(c["props"]["all_rows"]) == (2 if fused else 1)
    for n, q, m in c["props"]["mixed_rows"]:
        assert bad[n, q, m].any() and not bad[n, q, m].all()
        assert (out[n, q, m * D:(m + 1) * D] != 0).all()
    if fused:
        # the windowed kernel computes the last level's queries only: they hold every BAD value in x alone, in y alone and in both, in rows
        # whose other samples are ordinary, and one all-bad row
        last = c["props"]["last_level_start"]
        assert last == int(R.level_starts(c["shapes"])[-1]) and any(q >= last for _, q, _ in c["props"]["all_rows"])
        rl, bl = raw[:, last:], bad[:, last:]
        okf = lambda a: np.isfinite(a) & (np.abs(a) < 1e6)
        for sel in (~okf(rl[..., 0]) & okf(rl[..., 1]), okf(rl[..., 0]) & ~okf(rl[..., 1]), ~okf(rl[..., 0]) & ~okf(rl[..., 1])):
            assert not (sel & ~bl).any()
            vals = rl[sel]
            vals = vals[~okf(vals)]
            for b in R.BAD:
                assert (np.isnan(vals).any() if np.isnan(b) else (vals == np.float32(b)).any()), b
        assert sum(q >= last for _, q, _ in c["props"]["mixed_rows"]) == 21


def test_every_geometry_reaches_the_branch_it_is_named_for():
    want = {(8, 32, 4, 4): "fwd:shuffle_full", (8, 32, 4, 8): "bwd_loc:loops", (8, 32, 1, 1): "fwd:shuffle_one_slot", (8, 32, 2, 8): "fwd:shuffle_full",
            (3, 32, 2, 3): "bwd:M!=8", (1, 32, 3, 4): "bwd_loc:under_one_block", (16, 32, 3, 4): "bwd:M!=8",
            (8, 2, 3, 4): "fwd<1>", (8, 10, 3, 4): "fwd<1>", (8, 16, 3, 4): "fwd<4>:loops", (8, 64, 3, 4): "fwd<4>:loops"}
    union = set()
    for g in R.DROPIN_GEOMETRIES + R.DROPIN_FORWARD_ONLY:
        per = set()
        for Lq in R.DROPIN_LQ:
            per |= R.dropin_branches(*g, Lq, R.pyramid(g[2]))
        assert want[g] in per, g
        assert ("bwd:rejected" in per) == (g in R.DROPIN_FORWARD_ONLY)
        union |= per
    assert (8, 32, 4, 8) in R.DROPIN_GEOMETRIES and "fwd<4>:loops" in R.dropin_branches(8, 32, 4, 8, 5)        # L * P > 16 at D = 32
    assert "bwd_loc:under_one_block" in R.dropin_branches(8, 32, 4, 4, 1) and "level:H1_or_W1" in R.dropin_branches(8, 32, 4, 4, 1, R.pyramid(4))
    assert union == R.DROPIN_BRANCHES, union ^ R.DROPIN_BRANCHES
    assert all(h % 4 or w % 4 for h, w in R.pyramid(12))
    # fused forward: every branch of s2d_msda_fused_forward_f32 but the head-major experiment (ldv = -1, which ops.msda_fused_forward
    # cannot pass) is reached by a listed geometry or by the S2D geometry under one of the listed switches
    want_f = {(8, 4, 3): "tiled", (8, 2, 6): "tiled", (8, 1, 12): "tiled", (8, 12, 1): "rejected", (4, 3, 4): "share", (16, 3, 4): "share", (1, 3, 4): "share"}
    reached = set()
    for g in R.FUSED_GEOMETRIES:
        assert R.fused_branch(*g) == want_f[g], g
        reached.add(R.fused_branch(*g))
        reached.add(R.fused_branch(*g, env={"TILED": 0, "SHARE": 0}))
    sh = R.NONFINITE_PYRAMID
    S = sum(h * w for h, w in sh)
    for env in R.FUSED_ENVS:
        reached.add(R.fused_branch(8, 3, 4, env, sh, S))
    assert R.fused_branch(8, 3, 4, {"WIN": 1}, sh, S) == "win+tiled" and R.fused_branch(8, 3, 4, {"HEAD": 1}, sh, S) == "head"
    assert reached == R.FUSED_BRANCHES, reached ^ R.FUSED_BRANCHES
    assert sorted(l * p for l, p in R.TWO_STEP_LP) == [4, 8, 12, 16]
