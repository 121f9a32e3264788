"""MSDeformAttn kernels (csrc/msda.hip) on the inputs a continuous random draw never produces: samples on the pixel lattice and on
the -1 / H borders, non-finite and huge locations, cells holding 0 / 1 / 7 / 8 / 9 / 16 / 17 samples, and the geometries of the drop-in
op and of the fused forward that no other test runs.  References and cases: tests/msda_refs.py (proved on the CPU by
tests/test_msda_refs_cpu.py).

The rule (the project's own): max abs error relative to the largest reference element <= max(bound, 2 x the same figure of the
same expression in float32 torch on the device).  bound: 1e-5 forward (test_gpu_msda_glue.py), 2e-5 fused gradients
(test_gpu_backward.py), 1e-4 drop-in gradients (test_gpu_dropin.py).  Every row prints `msdarow <case> <form> <output> err torch32`.

S2D_MSDA_SHARE / S2D_MSDA_TILED are cached in the library on first use, so those forms run in a child process each (once per session,
every fused case in one child); S2D_MSDA_REC / WIN / HEAD are read per call."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import msda_refs as R

pytestmark = pytest.mark.gpu

FWD, FUSED_GRAD, DROPIN_GRAD = 1e-5, 2e-5, 1e-4
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _dev(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).cuda()


def _np(t):
    return t.detach().cpu().numpy()


def _err(got, ref, sel=None):
    ref = np.asarray(ref, np.float64)
    d = np.abs(np.asarray(got, np.float64) - ref)
    if sel is not None:
        d = d[sel]
    return float(d.max()) / max(float(np.abs(ref).max()), 1e-30) if d.size else 0.0


def rule(row, got, ref, t32, bound, sel=None):
    assert np.isfinite(np.asarray(got)).all(), row + ": NaN or inf"
    e, et = _err(got, ref, sel), _err(t32, ref, sel)
    print(f"msdarow {row} err {e:.2e} torch32 {et:.2e} bound {max(bound, 2 * et):.2e}")
    assert e <= max(bound, 2 * et), f"{row}: {e:.3e} > max({bound:.0e}, 2 x {et:.3e})"


def bits_zero(a):
    return not np.ascontiguousarray(a, np.float32).view(np.uint32).any()


def _shape_args(shapes):
    sh = np.array(shapes, np.int64)
    return sh, R.level_starts(shapes)


def dropin_forms(c, backward=True, f64=True):
    """-> {form: (out, grad_value, grad_loc, grad_attn)} (numpy; gradients None without backward)"""
    from s2d_amd import ops
    from s2d_amd.compat import MultiScaleDeformableAttention as msda_ext
    sh, ls = _shape_args(c["shapes"])
    sh_d, ls_d = torch.from_numpy(sh).cuda(), torch.from_numpy(ls).cuda()
    v, lo, a, go = _dev(c["value"]), _dev(c["loc"]), _dev(c["attn"]), _dev(c["grad_out"])
    res = {}
    out_h = ops.msda_forward(v, sh, ls, lo, a)
    out_d = ops.msda_forward_dev(v, sh_d, ls_d, lo, a)
    if not backward:
        return {"host": (_np(out_h), None, None, None), "dev": (_np(out_d), None, None, None)}
    res["sorted"] = (_np(out_h),) + tuple(_np(t) for t in ops.msda_backward(v, sh, ls, lo, a, go))
    res["atomic"] = (_np(out_h),) + tuple(_np(t) for t in ops.msda_backward(v, sh, ls, lo, a, go, atomics=True))
    res["dev"] = (_np(out_d),) + tuple(_np(t) for t in ops.msda_backward_dev(v, sh_d, ls_d, lo, a, go))
    if f64:
        v8, lo8, a8, go8 = (_dev(c[k], torch.float64) for k in ("value", "loc", "attn", "grad_out"))
        o8 = msda_ext.ms_deform_attn_forward(v8, sh_d, ls_d, lo8, a8, 64)
        res["f64"] = (_np(o8),) + tuple(_np(t) for t in msda_ext.ms_deform_attn_backward(v8, sh_d, ls_d, lo8, a8, go8, 64))
        msda_ext.check()
    return res


def torch32(c, backward=True):
    args = (_dev(c["value"]), c["shapes"], _dev(c["loc"]), _dev(c["attn"]))
    if not backward:
        return (_np(R.msda_torch(*args)), None, None, None)
    return tuple(_np(t) for t in R.msda_torch(*args, _dev(c["grad_out"])))


NAMES = ("out", "grad_value", "grad_loc", "grad_attn")


# --------------------------------------------------------------------------- lattice
@pytest.mark.parametrize("pyr,P", [("pow2", 4), ("pow2", 6), ("h1", 4), ("h1", 6), ("w1", 4), ("w1", 6)])
def test_lattice_dropin_equals_float64(pyr, P):
    """P = 4: the 8-lane set-up paths (L * P = 12); P = 6: sample_accum and the loops of msda_bwd_loc_kernel (L * P = 18).  Every output
    and gradient of every form, grad_loc at lattice and border samples included, EQUALS the float64 reference (exact in float32 in
    any order: test_lattice_case_is_exact_in_float32_in_any_order)."""
    c = R.lattice_case(pyr, P=P)
    ref = R.msda_ref(c["value"], c["shapes"], c["loc"], c["attn"], c["grad_out"])
    for form, got in dropin_forms(c).items():
        for g, r, name in zip(got, ref, NAMES):
            want = r if form == "f64" else r.astype(np.float32)
            bad = int((g != want).sum())
            print(f"msdarow lattice_{pyr}_P{P} {form} {name} unequal {bad} of {g.size}")
            assert g.shape == want.shape and bad == 0, (form, name, bad)


# --------------------------------------------------------------------------- fused forms: every fused case once per process
@functools.lru_cache(maxsize=None)
def fused_cases():
    d = {f"lattice_{p}": R.fused_lattice_case(p) for p in R.LATTICE_PYRAMIDS}
    d["offgrid"] = R.fused_lattice_case("offgrid", N=1)
    d["nonfinite"] = R.fused_nonfinite_case()
    for g in R.FUSED_GEOMETRIES:
        if R.fused_branch(*g) != "rejected":
            d["geom_%d_%d_%d" % g] = R.fused_geometry_case(*g)
    return d


def child_main(path):
    """the fused forward of every fused case with whatever S2D_MSDA_SHARE / S2D_MSDA_TILED this process was started under"""
    from s2d_amd import ops
    res = {}
    for name, c in fused_cases().items():
        res[name] = _np(ops.msda_fused_forward(_dev(c["value"]), np.array(c["shapes"], np.int64), _dev(c["oa"]), M=c["M"], P=c["P"]))
    torch.cuda.synchronize()
    np.savez(path, **res)


@pytest.fixture(scope="module")
def fused_ref64():
    return {name: R.fused_ref(c["value"], c["shapes"], c["oa"], c["M"], c["P"], c["grad_out"]) for name, c in fused_cases().items()}


@pytest.fixture(scope="module")
def fused_children(tmp_path_factory):
    """{("share" | "plain"): {case: out}}: S2D_MSDA_TILED=0 with S2D_MSDA_SHARE=1 / 0, set before the library loads"""
    res = {}
    for form, share in (("share", "1"), ("plain", "0")):
        path = str(tmp_path_factory.mktemp("msda_" + form) / "out.npz")
        env = dict(os.environ, S2D_MSDA_TILED="0", S2D_MSDA_SHARE=share)
        r = subprocess.run([sys.executable, "-c", "import sys; from tests.test_gpu_msda_edges import child_main; child_main(sys.argv[1])", path],
                           cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
        res[form] = dict(np.load(path))
    return res


def fused_forward_forms(c, monkeypatch):
    """in-process forms of the fused forward that the case's geometry admits -> {form: out}"""
    from s2d_amd import ops
    v, o, sh = _dev(c["value"]), _dev(c["oa"]), np.array(c["shapes"], np.int64)
    M, P, L = c["M"], c["P"], len(c["shapes"])
    S = c["value"].shape[1]
    res = {}
    for env in R.FUSED_ENVS:
        if "TILED" in env:
            continue
        branch = R.fused_branch(M, L, P, env, c["shapes"], S)
        if env and branch in res:
            continue                                                  # the switch does not apply to this geometry
        for k in ("REC", "WIN", "HEAD"):
            monkeypatch.delenv("S2D_MSDA_" + k, raising=False)
        for k, val in env.items():
            monkeypatch.setenv("S2D_MSDA_" + k, str(val))
        res[branch] = _np(ops.msda_fused_forward(v, sh, o, M=M, P=P))
    for k in ("REC", "WIN", "HEAD"):
        monkeypatch.delenv("S2D_MSDA_" + k, raising=False)
    return res


def fused_torch32(c):
    return tuple(_np(t) for t in R.fused_torch(_dev(c["value"]), c["shapes"], _dev(c["oa"]), c["M"], c["P"], _dev(c["grad_out"])))


def fused_backward_forms(c):
    from s2d_amd import backward
    v, o, go, sh = _dev(c["value"]), _dev(c["oa"]), _dev(c["grad_out"]), np.array(c["shapes"], np.int64)
    res = {}
    assert backward._MSDA_BWD_REC
    for form, flag in (("rec", True), ("two_step", False)):
        backward._MSDA_BWD_REC = flag
        try:
            res[form] = tuple(_np(t) for t in backward.msda_fused_backward(v, sh, o, go, M=c["M"], P=c["P"]))
        finally:
            backward._MSDA_BWD_REC = True
    return res


def _fused_check(tag, c, ref, forms, children, bwd, identical=True):
    out64, gv64, doa64 = ref
    t_out, t_gv, t_doa = fused_torch32(c)
    M, P, L = c["M"], c["P"], len(c["shapes"])
    allf = dict(forms)
    for form, outs in children.items():
        allf["child_" + form] = outs
    first = None
    for form, out in allf.items():
        rule(f"{tag} {form} out", out, out64, t_out, FWD)
        if identical:
            first = out if first is None else first
            assert np.array_equal(out.view(np.uint32), first.view(np.uint32)), f"{tag}: {form} differs in bits from {next(iter(allf))}"
    # the offset gradient of a sample the range test skips is 0 in the reference; torch's grid_sample has no range test and differs at
    # exactly -1, so torch's figure is taken over the samples inside the maps only
    inside = R.cells_fused(c["oa"], c["shapes"], M, P, np.float64)[0]
    N, S = inside.shape[:2]
    sel = np.concatenate([np.repeat(inside.reshape(N, S, -1), 2, -1), np.ones((N, S, M * L * P), bool)], -1)
    for form, (gv, doa) in bwd.items():
        rule(f"{tag} bwd_{form} d_value", gv, gv64, t_gv, FUSED_GRAD)
        assert np.isfinite(doa).all()
        e, et = _err(doa, doa64), _err(t_doa, doa64, sel)
        print(f"msdarow {tag} bwd_{form} d_offs_logits err {e:.2e} torch32 {et:.2e}")
        assert e <= max(FUSED_GRAD, 2 * et), (tag, form, e, et)
    return allf


@pytest.mark.parametrize("pyr", list(R.LATTICE_PYRAMIDS))
def test_lattice_fused_forms(pyr, fused_ref64, fused_children, monkeypatch):
    """every sample of the fused forms on a lattice / border target of a power-of-two level (the float32 cell is the float64 cell:
    test_fused_lattice_case_selects_the_float64_cells_in_float32), so every element of the offset gradient is compared too"""
    name = "lattice_" + pyr
    c = fused_cases()[name]
    forms = fused_forward_forms(c, monkeypatch)
    assert "rec8" in forms and "tiled" in forms and "rec4" in forms and "head" in forms
    _fused_check(name, c, fused_ref64[name], forms, {k: v[name] for k, v in fused_children.items()}, fused_backward_forms(c))


# --------------------------------------------------------------------------- offgrid
def test_offgrid_dropin():
    c = R.offgrid_case()
    sh = c["shapes"]
    ref = R.msda_ref(c["value"], sh, c["loc"], c["attn"], c["grad_out"])
    t32 = torch32(c)
    diff, free_share, delib_share = R.offgrid_disagreement(c)
    d = c["props"]["deliberate"]
    print(f"msdarow offgrid excluded share of free samples {free_share:.2e} (float32 cell != float64 cell); of deliberate lattice samples {delib_share:.3f}")
    assert free_share <= 1e-3
    (hh, wh), (hl, wl) = R.adjacent_cells(c["props"]["targets"])
    i64, h64, w64, _, _ = R.cells(c["loc"], sh)
    pick = lambda a, b: np.where(d, a, b)
    hi = R.msda_ref(c["value"], sh, c["loc"], c["attn"], c["grad_out"], cell=(pick(hh, np.where(i64, h64, -9)), pick(wh, np.where(i64, w64, -9))))[2]
    lo = R.msda_ref(c["value"], sh, c["loc"], c["attn"], c["grad_out"], cell=(pick(hl, np.where(i64, h64, -9)), pick(wl, np.where(i64, w64, -9))))[2]
    scale = np.abs(ref[2]).max()
    for form, got in dropin_forms(c).items():
        for k in (0, 1, 3):                                          # continuous across the lattice: every element
            rule(f"offgrid {form} {NAMES[k]}", got[k], ref[k], t32[k], FWD if k == 0 else DROPIN_GRAD)
        gl = got[2]
        assert np.isfinite(gl).all()
        keep = ~d & ~diff
        e_free = _err(gl, ref[2], np.broadcast_to(keep[..., None], gl.shape))
        et = _err(t32[2], ref[2], np.broadcast_to(keep[..., None], gl.shape))
        # a deliberate lattice sample: the one-sided value of one of the two cells adjacent to its lattice point, per component
        e_del = float((np.minimum(np.abs(gl - hi), np.abs(gl - lo))[d]).max() / scale)
        print(f"msdarow offgrid {form} grad_loc free err {e_free:.2e} torch32 {et:.2e}; deliberate (nearer adjacent cell) err {e_del:.2e}")
        assert e_free <= max(DROPIN_GRAD, 2 * et)
        assert e_del <= DROPIN_GRAD


def test_offgrid_fused_forms(fused_ref64, fused_children, monkeypatch):
    """every sample of the fused forms a float32 rounding away from a lattice / border target of a 5 x 9 / 11 x 19 / 23 x 37 level: out,
    d_value and the logit gradients are continuous across the lattice and compared on every element; an offset gradient is compared
    with float64 where the float32 cell is the float64 cell, and everywhere with the one-sided value of the nearer of the two cells
    adjacent to the sample's lattice point"""
    c = fused_cases()["offgrid"]
    M, P, L = c["M"], c["P"], len(c["shapes"])
    out64, gv64, doa64 = fused_ref64["offgrid"]
    t_out, t_gv, t_doa = fused_torch32(c)
    forms = fused_forward_forms(c, monkeypatch)
    forms.update({"child_" + k: v["offgrid"] for k, v in fused_children.items()})
    first = next(iter(forms.values()))
    for form, out in forms.items():
        rule(f"offgrid_fused {form} out", out, out64, t_out, FWD)
        assert np.array_equal(out.view(np.uint32), first.view(np.uint32)), form
    diff = R.fused_offgrid_disagreement(c)
    print(f"msdarow offgrid_fused float32 cell != float64 cell on {diff.mean():.3f} of the samples (all deliberate)")
    hi_c, lo_c = R.adjacent_cells(c["props"]["targets"])
    noff = M * L * P * 2
    hi = R.fused_ref(c["value"], c["shapes"], c["oa"], M, P, c["grad_out"], cell=hi_c)[2][..., :noff]
    lo = R.fused_ref(c["value"], c["shapes"], c["oa"], M, P, c["grad_out"], cell=lo_c)[2][..., :noff]
    N, S = diff.shape[:2]
    same = np.repeat((~diff).reshape(N, S, -1), 2, -1)
    scale = np.abs(doa64[..., :noff]).max()
    for form, (gv, doa) in fused_backward_forms(c).items():
        rule(f"offgrid_fused bwd_{form} d_value", gv, gv64, t_gv, FUSED_GRAD)
        rule(f"offgrid_fused bwd_{form} d_logits", doa[..., noff:], doa64[..., noff:], t_doa[..., noff:], FUSED_GRAD)
        goff = doa[..., :noff]
        assert np.isfinite(goff).all()
        e_same = float(np.abs(goff - doa64[..., :noff])[same].max() / scale)
        e_near = float(np.minimum(np.abs(goff - hi), np.abs(goff - lo)).max() / scale)
        print(f"msdarow offgrid_fused bwd_{form} d_offsets where the cells agree err {e_same:.2e}; every sample, nearer adjacent cell err {e_near:.2e}")
        assert e_same <= FUSED_GRAD and e_near <= FUSED_GRAD


# --------------------------------------------------------------------------- nonfinite
def test_nonfinite_dropin():
    c = R.nonfinite_case()
    ref = R.msda_ref(c["value"], c["shapes"], c["loc"], c["attn"], c["grad_out"])
    t32 = torch32(c)
    bad = c["props"]["bad"]
    (n, q, m), = c["props"]["all_rows"]
    D = c["value"].shape[-1]
    for form, got in dropin_forms(c).items():
        for k in range(4):
            rule(f"nonfinite {form} {NAMES[k]}", got[k], ref[k], t32[k], FWD if k == 0 else DROPIN_GRAD)
        assert (got[2][bad] == 0).all() and (got[3][bad] == 0).all(), form
        if form != "f64":
            assert bits_zero(got[0][n, q, m * D:(m + 1) * D]), form
        assert (got[0][n, q, m * D:(m + 1) * D] == 0).all()


def test_nonfinite_fused_forms_agree_bit_for_bit(fused_ref64, fused_children, monkeypatch):
    """a NaN / +-inf / 1e30 / 3e9 raw offset: the sample is skipped (cuh:293), the rest of its row stays finite, the row with nothing
    but such samples is bitwise 0, and the record forms, the TILED / SHARE / plain forms, the windowed and the head-per-workgroup
    kernels give the same bits.  The poisoned rows lie on level 0 and on the last level: under S2D_MSDA_WIN=1 the windowed kernel
    computes the last level's queries and the TILED kernel the others."""
    c = fused_cases()["nonfinite"]
    forms = fused_forward_forms(c, monkeypatch)
    assert set(forms) == {"rec8", "rec4", "tiled", "win+tiled", "head"}
    bwd = fused_backward_forms(c)
    allf = _fused_check("nonfinite_fused", c, fused_ref64["nonfinite"], forms, {k: v["nonfinite"] for k, v in fused_children.items()}, bwd)
    last = c["props"]["last_level_start"]                                  # the windowed kernel computes the queries q >= last only
    assert any(q >= last for _, q, _ in c["props"]["all_rows"]) and any(q >= last for _, q, _ in c["props"]["mixed_rows"])
    for form, out in allf.items():
        for n, q, m in c["props"]["all_rows"]:
            assert bits_zero(out[n, q, m * 32:(m + 1) * 32]), (form, q)
    bad = c["props"]["bad"]
    N, S = bad.shape[:2]
    for form, (gv, doa) in bwd.items():
        goff = doa[..., :8 * 12 * 2].reshape(N, S, 8, 3, 4, 2)
        assert (goff[bad] == 0).all(), form


# --------------------------------------------------------------------------- segments
def test_segments_grad_value():
    from s2d_amd import ops
    for kind in ("counts", "one_cell", "corners", "all_outside"):
        c = R.segments_case(kind)
        sh, ls = _shape_args(c["shapes"])
        sh_d, ls_d = torch.from_numpy(sh).cuda(), torch.from_numpy(ls).cuda()
        v, lo, a, go = _dev(c["value"]), _dev(c["loc"]), _dev(c["attn"]), _dev(c["grad_out"])
        ref = R.msda_ref(c["value"], c["shapes"], c["loc"], c["attn"], c["grad_out"])[1]
        t32 = torch32(c)[1]
        g1 = ops.msda_backward(v, sh, ls, lo, a, go)[0]
        g2 = ops.msda_backward(v, sh, ls, lo, a, go)[0]
        gd = ops.msda_backward_dev(v, sh_d, ls_d, lo, a, go)[0]
        ga = ops.msda_backward(v, sh, ls, lo, a, go, atomics=True)[0]
        assert torch.equal(g1, g2), kind + ": the sorted backward is not reproducible"
        assert torch.equal(g1, gd), kind + ": host-shape and device-shape forms differ"
        rule(f"segments_{kind} sorted grad_value", _np(g1), ref, t32, DROPIN_GRAD)
        rule(f"segments_{kind} atomic grad_value", _np(ga), ref, t32, DROPIN_GRAD)
        e = _err(_np(ga), _np(g1).astype(np.float64))
        print(f"msdarow segments_{kind} sorted vs atomic {e:.2e}")
        assert e <= DROPIN_GRAD
        if kind == "all_outside":
            assert not np.abs(ref).any() and bits_zero(_np(g1)) and bits_zero(_np(ga)) and bits_zero(_np(gd))
        if kind == "counts":
            assert np.abs(ref[0, :, 0]).max() > 0


# --------------------------------------------------------------------------- geometries
@pytest.mark.parametrize("geom", R.DROPIN_GEOMETRIES + R.DROPIN_FORWARD_ONLY, ids=lambda g: "M%d_D%d_L%d_P%d" % g)
def test_geometries_dropin(geom):
    from s2d_amd import ops
    from s2d_amd.compat import MultiScaleDeformableAttention as msda_ext
    M, D, L, P = geom
    backward = D == 32
    for Lq in R.DROPIN_LQ:
        c = R.geometry_case(M, D, L, P, Lq)
        ref = R.msda_ref(c["value"], c["shapes"], c["loc"], c["attn"], c["grad_out"] if backward else None)
        if not backward:
            ref = (ref, None, None, None)
        t32 = torch32(c, backward)
        for form, got in dropin_forms(c, backward, f64=False).items():
            for k in range(4 if backward else 1):
                rule(f"geom_M{M}_D{D}_L{L}_P{P}_Lq{Lq} {form} {NAMES[k]}", got[k], ref[k], t32[k], FWD if k == 0 else DROPIN_GRAD)
        if not backward:
            # the float32 backward exists for D = 32 only: it must raise, not run
            sh, ls = _shape_args(c["shapes"])
            sh_d, ls_d = torch.from_numpy(sh).cuda(), torch.from_numpy(ls).cuda()
            v, lo, a, go = _dev(c["value"]), _dev(c["loc"]), _dev(c["attn"]), _dev(c["grad_out"])
            for call in (lambda: ops.msda_backward(v, sh, ls, lo, a, go), lambda: ops.msda_backward(v, sh, ls, lo, a, go, atomics=True),
                         lambda: ops.msda_backward_dev(v, sh_d, ls_d, lo, a, go),
                         lambda: msda_ext.ms_deform_attn_backward(v, sh_d, ls_d, lo, a, go, 64)):
                with pytest.raises(RuntimeError):
                    call()


@pytest.mark.parametrize("geom", R.FUSED_GEOMETRIES, ids=lambda g: "M%d_L%d_P%d" % g)
def test_geometries_fused_forward(geom, fused_ref64, fused_children, monkeypatch):
    from s2d_amd import ops
    M, L, P = geom
    if R.fused_branch(M, L, P) == "rejected":
        # L = 12 is more levels than the kernels' level table holds (MAX_L = 8): the entry point must refuse, not run
        c = R.fused_geometry_case(M, L, P)
        with pytest.raises(RuntimeError):
            ops.msda_fused_forward(_dev(c["value"]), np.array(c["shapes"], np.int64), _dev(c["oa"]), M=M, P=P)
        return
    name = "geom_%d_%d_%d" % geom
    c = fused_cases()[name]
    forms = fused_forward_forms(c, monkeypatch)
    assert R.fused_branch(M, L, P) in forms
    out64 = fused_ref64[name][0]
    t_out = _np(R.fused_torch(_dev(c["value"]), c["shapes"], _dev(c["oa"]), M, P))
    forms.update({"child_" + k: v[name] for k, v in fused_children.items()})
    first = next(iter(forms.values()))
    for form, out in forms.items():
        rule(f"{name} {form} out", out, out64, t_out, FWD)
        assert np.array_equal(out.view(np.uint32), first.view(np.uint32)), form
    # and the backward the module would run at this geometry (the two-step form: the record form is for M = 8, L = 3, P = 4 only)
    from s2d_amd import backward
    _, t_gv, t_doa = fused_torch32(c)
    gv, doa = backward.msda_fused_backward(_dev(c["value"]), np.array(c["shapes"], np.int64), _dev(c["oa"]), _dev(c["grad_out"]), M=M, P=P)
    rule(f"{name} backward d_value", _np(gv), fused_ref64[name][1], t_gv, FUSED_GRAD)
    rule(f"{name} backward d_offs_logits", _np(doa), fused_ref64[name][2], t_doa, FUSED_GRAD)


@pytest.mark.parametrize("L,P", R.TWO_STEP_LP)
@pytest.mark.parametrize("M", [8, 4])
def test_two_step_fused_backward_every_sample_count(L, P, M):
    """s2d_msda_fused_prep_f32 / chain accept L * P in 4, 8, 12, 16; only 12 had a test"""
    from s2d_amd import backward
    c = R.fused_geometry_case(M, L, P)
    out64, gv64, doa64 = R.fused_ref(c["value"], c["shapes"], c["oa"], M, P, c["grad_out"])
    _, t_gv, t_doa = fused_torch32(c)
    backward._MSDA_BWD_REC = False
    try:
        gv, doa = backward.msda_fused_backward(_dev(c["value"]), np.array(c["shapes"], np.int64), _dev(c["oa"]), _dev(c["grad_out"]), M=M, P=P)
    finally:
        backward._MSDA_BWD_REC = True
    rule(f"two_step_M{M}_L{L}_P{P} d_value", _np(gv), gv64, t_gv, FUSED_GRAD)
    rule(f"two_step_M{M}_L{L}_P{P} d_offs_logits", _np(doa), doa64, t_doa, FUSED_GRAD)
