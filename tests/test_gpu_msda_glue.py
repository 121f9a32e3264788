"""GPU parity: MSDeformAttn kernels and the bandwidth-bound glue kernels vs goldens / the CPU oracle."""
import numpy as np
import pytest
import torch

from s2d_amd.utils import synth
from tests.conftest import golden

pytestmark = pytest.mark.gpu


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def close(a, b, rtol):
    b = np.asarray(b, np.float64)
    np.testing.assert_allclose(np.asarray(a, np.float64), b, rtol=rtol, atol=rtol * max(np.abs(b).max(), 1e-30))


def test_msda_optest_fixture(oracle):
    """the reference's only known-answer test (ops/test.py:24-31,51-63), D=2 -> scalar path"""
    from s2d_amd import ops
    g = golden("msda_optest")
    lsi = oracle.level_start_index(g["shapes"])
    out = ops.msda_forward(_dev(g["value"]), g["shapes"], lsi, _dev(g["loc"]), _dev(g["w"])).cpu().numpy()
    np.testing.assert_allclose(out, g["out32"], rtol=1e-2, atol=1e-3)     # the reference's own tolerance
    np.testing.assert_allclose(out, g["out64"], rtol=1e-5, atol=1e-7)


def test_msda_forward_backward_golden(oracle):
    from s2d_amd import ops
    g = golden("msda_core")
    lsi = oracle.level_start_index(g["shapes"])
    v, lo, w = _dev(g["value"]), _dev(g["loc"]), _dev(g["w"])
    out = ops.msda_forward(v, g["shapes"], lsi, lo, w).cpu().numpy()
    close(out, g["out"], 1e-5)
    gv, gl, gw = ops.msda_backward(v, g["shapes"], lsi, lo, w, _dev(g["grad_out"]))
    close(gv.cpu().numpy(), g["grad_value"], 1e-4)
    close(gl.cpu().numpy(), g["grad_loc"], 1e-4)
    close(gw.cpu().numpy(), g["grad_w"], 1e-4)


@pytest.mark.parametrize("shapes,N", [([(6, 10), (12, 20), (23, 40)], 2), ([(23, 40), (46, 80), (92, 160)], 1)],
                         ids=["quarter_size_pyramid", "720p_pyramid"])
def test_msda_fused_vs_oracle_720p_shapes(oracle, shapes, N):
    """fused softmax+loc+gather against the oracle's module arithmetic: a quarter-size pyramid (two frames) and the real pyramid of
    a 736 x 1280 frame -- (23,40), (46,80), (92,160), S = 19 320 queries per frame, the benched geometry"""
    from s2d_amd import ops
    S = sum(h * w for h, w in shapes)
    M, D, L, P = 8, 32, 3, 4
    value = synth.randn(7, 1, (N, S, M * D))
    off = synth.randn(7, 2, (N, S, M, L, P, 2), 2.0)
    lg = synth.randn(7, 3, (N, S, M, L * P))
    oa = np.concatenate([off.reshape(N, S, -1), lg.reshape(N, S, -1)], -1)
    ref_pts = oracle.reference_points(shapes)
    norm = np.array([[w_, h_] for (h_, w_) in shapes], np.float32)
    loc = ref_pts[None, :, None, :, None, :] + off / norm[None, None, None, :, None, :]
    aw = oracle.softmax(lg, -1).reshape(N, S, M, L, P)
    ref = oracle.msda_core(value.reshape(N, S, M, D), np.array(shapes), oracle.level_start_index(shapes),
                           loc.astype(np.float32), aw.astype(np.float32))
    out = ops.msda_fused_forward(_dev(value), np.array(shapes), _dev(oa)).cpu().numpy()
    close(out, ref, 1e-5)
    # value / offsets+logits as column slices of one [N,S,288+256] buffer (the merged projection's output)
    both = _dev(np.concatenate([oa, value], -1))
    out1 = ops.msda_fused_forward(both[..., oa.shape[-1]:], np.array(shapes), both[..., :oa.shape[-1]]).cpu().numpy()
    assert np.array_equal(out1, out)
    # and the drop-in form on the same data
    out2 = ops.msda_forward(_dev(value.reshape(N, S, M, D)), np.array(shapes), oracle.level_start_index(shapes),
                            _dev(loc.astype(np.float32)), _dev(aw.astype(np.float32))).cpu().numpy()
    close(out2, ref, 1e-5)


def test_msda_windowed_kernel_opt_in_matches_the_gather_kernel(oracle, monkeypatch):
    """the opt-in LDS-windowed fused kernel (S2D_MSDA_WIN=1) against the oracle and bit for bit against the default gather kernel:
    offsets inside the windows (branch-free path), scattered beyond them (general path), border patches overhanging a level whose
    extent is not a multiple of 8, and column-slice operands"""
    import torch
    from s2d_amd import ops
    for shapes, scale in (([(6, 10), (12, 20), (23, 40)], 2.0), ([(5, 9), (11, 19), (22, 37)], 0.4), ([(6, 10), (12, 20), (23, 40)], 8.0)):
        S = sum(h * w for h, w in shapes)
        N, M, D, L, P = 2, 8, 32, 3, 4
        value = synth.randn(11, 1, (N, S, M * D))
        off = synth.randn(11, 2, (N, S, M, L, P, 2), scale)
        lg = synth.randn(11, 3, (N, S, M, L * P))
        oa = np.concatenate([off.reshape(N, S, -1), lg.reshape(N, S, -1)], -1)
        both = _dev(np.concatenate([oa, value], -1))
        v, o = both[..., oa.shape[-1]:], both[..., :oa.shape[-1]]
        monkeypatch.setenv("S2D_MSDA_WIN", "0")
        base = ops.msda_fused_forward(v, np.array(shapes), o)
        monkeypatch.setenv("S2D_MSDA_WIN", "1")
        win = ops.msda_fused_forward(v, np.array(shapes), o)
        assert torch.equal(win, base)
        ref_pts = oracle.reference_points(shapes)
        norm = np.array([[w_, h_] for (h_, w_) in shapes], np.float32)
        loc = ref_pts[None, :, None, :, None, :] + off / norm[None, None, None, :, None, :]
        aw = oracle.softmax(lg, -1).reshape(N, S, M, L, P)
        ref = oracle.msda_core(value.reshape(N, S, M, D), np.array(shapes), oracle.level_start_index(shapes), loc.astype(np.float32), aw.astype(np.float32))
        close(win.cpu().numpy(), ref, 1e-5)


def test_msda_head_per_workgroup_kernel_matches_the_patch_kernel(oracle, monkeypatch):
    """the opt-in fused kernel with one head per workgroup and the coarsest level's plane of that head in LDS (S2D_MSDA_HEAD=1)
    bit for bit against the default 4 x 4-patch gather kernel and against the oracle: level extents that are /
    are not multiples of the 16 x 8 query patch, the coarsest level first / last / in the middle, offsets within a pixel and far
    outside the maps (zero-padding corners), column-slice operands, one frame and several"""
    import torch
    from s2d_amd import ops
    cases = (([(6, 10), (12, 20), (23, 40)], 2.0, 2), ([(23, 40), (46, 80), (92, 160)], 3.0, 1), ([(22, 37), (5, 9), (11, 19)], 0.4, 3),
             ([(8, 16), (16, 32), (3, 5)], 30.0, 2))
    for shapes, scale, N in cases:
        S = sum(h * w for h, w in shapes)
        M, D, L, P = 8, 32, 3, 4
        value = synth.randn(21, 1, (N, S, M * D))
        off = synth.randn(21, 2, (N, S, M, L, P, 2), scale)
        lg = synth.randn(21, 3, (N, S, M, L * P))
        oa = np.concatenate([off.reshape(N, S, -1), lg.reshape(N, S, -1)], -1)
        both = _dev(np.concatenate([oa, value], -1))
        v, o = both[..., oa.shape[-1]:], both[..., :oa.shape[-1]]
        monkeypatch.setenv("S2D_MSDA_HEAD", "0")
        base = ops.msda_fused_forward(v, np.array(shapes), o)
        monkeypatch.setenv("S2D_MSDA_HEAD", "1")
        head = ops.msda_fused_forward(v, np.array(shapes), o)
        assert torch.equal(head, base)
        ref_pts = oracle.reference_points(shapes)
        norm = np.array([[w_, h_] for (h_, w_) in shapes], np.float32)
        loc = ref_pts[None, :, None, :, None, :] + off / norm[None, None, None, :, None, :]
        aw = oracle.softmax(lg, -1).reshape(N, S, M, L, P)
        ref = oracle.msda_core(value.reshape(N, S, M, D), np.array(shapes), oracle.level_start_index(shapes), loc.astype(np.float32), aw.astype(np.float32))
        close(head.cpu().numpy(), ref, 1e-5)


def test_normalize_pad_maxpool(oracle):
    from s2d_amd import ops
    fr = synth.smooth_frames_u8(3, 1, 2, 45, 70)
    ref = oracle.normalize_pad(fr)                       # [F,3,Hp,Wp]
    out = ops.normalize_pad(_dev(fr)).cpu().numpy()
    assert out.shape == (2, 64, 96, 4)
    close(out[..., :3].transpose(0, 3, 1, 2), ref, 1e-6)
    assert (out[..., 3] == 0).all()
    x = synth.randn(3, 2, (2, 64, 17, 23))
    y = ops.maxpool3x3s2(_dev(x.transpose(0, 2, 3, 1))).cpu().numpy().transpose(0, 3, 1, 2)
    np.testing.assert_array_equal(y, oracle.max_pool_3x3_s2_p1(x))


def test_groupnorm_layernorm_add_pe(oracle):
    from s2d_amd import ops
    x = synth.randn(4, 1, (2, 256, 12, 20)) * 3 + 1
    ga, be = synth.randn(4, 2, (256,)) * 0.1 + 1, synth.randn(4, 3, (256,)) * 0.1
    ref = oracle.group_norm(x, 32, ga, be)
    xd = _dev(x.transpose(0, 2, 3, 1))
    y = ops.groupnorm_nhwc(xd, 32, _dev(ga), _dev(be)).cpu().numpy().transpose(0, 3, 1, 2)
    close(y, ref, 1e-5)
    up = synth.randn(4, 4, (2, 256, 6, 10))
    ref2 = np.maximum(ref + oracle.resize_bilinear(up, 12, 20), 0)
    y2 = ops.groupnorm_nhwc(xd, 32, _dev(ga), _dev(be), up=_dev(up.transpose(0, 2, 3, 1)), relu=True)
    close(y2.cpu().numpy().transpose(0, 3, 1, 2), ref2, 1e-5)
    # layernorm(x + res)
    a, r = synth.randn(4, 5, (3, 50, 256)), synth.randn(4, 6, (3, 50, 256))
    close(ops.layernorm(_dev(a), _dev(ga), _dev(be), res=_dev(r)).cpu().numpy(), oracle.layer_norm(a + r, ga, be), 1e-5)
    # broadcast add
    b = synth.randn(4, 7, (50, 256))
    close(ops.add_bcast(_dev(a), _dev(b)).cpu().numpy(), a + b[None], 1e-7)
    # position encodings vs the reference goldens
    g = golden("pe")
    pe2 = ops.pe_sine(0, 5, 7).cpu().numpy().reshape(5, 7, 256).transpose(2, 0, 1)
    np.testing.assert_allclose(pe2, g["pe2"][0], rtol=0, atol=2e-5)
    pe3 = ops.pe_sine(3, 4, 6).cpu().numpy().reshape(3, 4, 6, 256).transpose(0, 3, 1, 2)
    np.testing.assert_allclose(pe3, g["pe3"][0], rtol=0, atol=2e-5)


def test_msda_backward_sorted_is_reproducible_and_matches_the_atomic_form():
    """the training step's MSDeformAttn backward (sampling graph inverted by a stable sort, grad_value rows gathered) against
    the reference-style scatter with float atomics on a 3-level pyramid with offsets that leave the maps: same gradients
    (the two differ only in summation order), and the sorted form is bitwise identical run to run"""
    import torch
    from s2d_amd import ops
    shapes = np.array([(12, 20), (23, 40), (46, 80)])
    S = int((shapes[:, 0] * shapes[:, 1]).sum())
    N, M, D, L, P = 3, 8, 32, 3, 4
    g = torch.Generator().manual_seed(11)
    value = torch.randn((N, S, M, D), generator=g).cuda()
    loc = (torch.rand((N, S, M, L, P, 2), generator=g) * 1.3 - 0.15).cuda()          # some samples outside [0, 1]
    loc[0, :50] = 0.5                                                               # a hot cell: hundreds of samples on one pixel
    aw = torch.softmax(torch.randn((N, S, M, L * P), generator=g), -1).view(N, S, M, L, P).cuda()
    go = torch.randn((N, S, M * D), generator=g).cuda()
    lsi = np.concatenate([[0], np.cumsum(shapes[:, 0] * shapes[:, 1])[:-1]])
    a = ops.msda_backward(value, shapes, lsi, loc, aw, go)
    b = ops.msda_backward(value, shapes, lsi, loc, aw, go)
    c = ops.msda_backward(value, shapes, lsi, loc, aw, go, atomics=True)
    for x, y, z, name in zip(a, b, c, ("grad_value", "grad_loc", "grad_attn")):
        assert torch.equal(x, y), name
        scale = float(z.abs().max())
        assert float((x - z).abs().max()) <= 2e-5 * scale, name


# --------------------------------------------------------------------------- both sides of the element-wise kernels' size thresholds
def _rel64(got, ref):
    """`rel` of tests/test_gpu_backward.py on device tensors: max abs error / max abs reference"""
    return float((got.double() - ref).abs().max()) / max(float(ref.abs().max()), 1e-30)


def _groupnorm64(x, G, ga, be, up=None, relu=False, dt=torch.float64):
    """float64 GroupNorm (+ bilinear `up`, ReLU) of an NHWC float32 tensor, in plain torch on the device"""
    F = torch.nn.functional
    y = F.group_norm(x.to(dt).permute(0, 3, 1, 2), G, ga.to(dt), be.to(dt), 1e-5)
    if up is not None:
        y = y + F.interpolate(up.to(dt).permute(0, 3, 1, 2), size=tuple(x.shape[1:3]), mode="bilinear", align_corners=False)
    y = y.permute(0, 2, 3, 1)
    return torch.relu(y) if relu else y


# HW = 257 / 258: two row blocks of gn_stats_kernel (256 rows each at HW <= 61 440), the last one ragged with 1 / 2 rows;
# 62 x 1000 = 62 000 = 4 k: rows_per_blk = 259, 240 blocks, last block 99 rows, gn_reduce_kernel lanes with 3 and 4 partials;
# N * HW * C / 4 around 2^20 at C = 256 and N = 4: HW = 4096 (exactly 2^20, gn_apply_px_kernel), 4092 (HW % 4 == 0 just below, gn_apply_kernel),
# 4094 and 4102 (HW % 4 == 2 just below and just above: gn_apply_kernel on both sides); C = 64 and C = 1024 on both sides as well
_GN_CASES = [(2, 1, 257, 256, None), (2, 129, 2, 256, None), (1, 62, 1000, 256, (31, 500)), (4, 64, 64, 256, (32, 32)), (4, 62, 66, 256, None),
             (4, 46, 89, 256, None), (4, 2, 2051, 256, (1, 1025)), (2, 46, 45, 256, (23, 45)), (3, 45, 46, 256, (23, 23)),
             (16, 64, 64, 64, (32, 32)), (15, 64, 64, 64, None), (1, 64, 64, 1024, (32, 32)), (1, 62, 66, 1024, None), (1, 3, 86, 1024, None)]


@pytest.mark.parametrize("N,H,W,C,up_hw", _GN_CASES)
def test_groupnorm_both_sides_of_the_size_thresholds(N, H, W, C, up_hw):
    """groupnorm_nhwc against float64 torch at 1e-5 (the bound of test_groupnorm_layernorm_add_pe): several row blocks with a ragged
    last one, both apply kernels on both sides of the 2^20 threshold, `up` maps that are and are not exactly half the size, with and
    without ReLU, and a group whose mean is 1e3 x its standard deviation (group 1: the double-precision statistics keep its variance)"""
    from s2d_amd import ops
    g = torch.Generator(device="cuda").manual_seed(N * 1000003 + H * 1009 + W * 31 + C)
    G = 32 if C >= 128 else 8                 # groups hold a multiple of 4 channels
    x = torch.randn((N, H, W, C), device="cuda", generator=g) * 3 + 1
    cg = C // G
    x[..., cg:2 * cg] = torch.randn((N, H, W, cg), device="cuda", generator=g) + 1000.0
    ga = torch.randn((C,), device="cuda", generator=g) * 0.1 + 1
    be = torch.randn((C,), device="cuda", generator=g) * 0.1
    def check(y, ref, tag, up_err=0.0):
        # 1e-5 of the output scale on the whole tensor, and 1e-5 of ITS OWN scale on the offset group alone (the kernel keeps the statistics
        # in double; measured on that group: at most 6.8e-6, which is the float32 rounding of a mean of 1e3 against a deviation of 1).
        # With `up`: the source position of a tap is formed in float32 (by the kernel as by torch), a few units of 2^-24 of a coordinate
        # that reaches 1 025 in the 2 x 2051 case, times the difference of neighbouring taps -- there the rule of
        # tests/test_gpu_forward_c4.py holds for that term alone: max(1e-5, 2 x the error of torch's float32 interpolation of `up` against its
        # float64 one, up_err, as a share of the output scale); the normalisation gets no allowance from float32 torch
        r, r1 = _rel64(y, ref), _rel64(y[..., cg:2 * cg], ref[..., cg:2 * cg])
        top, top1 = float(ref.abs().max()), float(ref[..., cg:2 * cg].abs().max())
        print(f"groupnorm {N}x{H}x{W}x{C} {tag}: rel {r:.3e}, offset group alone {r1:.3e}, float32 interpolation error {up_err:.3e}")
        assert r < max(1e-5, 2.0 * up_err / top) and r1 < max(1e-5, 2.0 * up_err / top1)

    y = ops.groupnorm_nhwc(x, G, ga, be)
    assert torch.equal(y, ops.groupnorm_nhwc(x, G, ga, be))
    check(y, _groupnorm64(x, G, ga, be), "plain")
    if up_hw is not None:
        up = torch.randn((N, up_hw[0], up_hw[1], C), device="cuda", generator=g)
        interp = lambda t: torch.nn.functional.interpolate(t.permute(0, 3, 1, 2), size=(H, W), mode="bilinear", align_corners=False)
        up_err = float((interp(up).double() - interp(up.double())).abs().max())
        for relu in (False, True):
            y2 = ops.groupnorm_nhwc(x, G, ga, be, up=up, relu=relu)
            check(y2, _groupnorm64(x, G, ga, be, up, relu), "up relu" if relu else "up", up_err)
            if relu:
                assert float(y2.min()) >= 0.0


@pytest.mark.parametrize("rows", [4095, 4096, 4097, 4098, 4099, 4111])
@pytest.mark.parametrize("with_res", [False, True])
def test_layernorm_both_kernels_and_every_tail(rows, with_res):
    """C = 256: layernorm_kernel below 4096 rows, layernorm256_kernel<4> from there (16 rows per workgroup, a wave's last rows recomputed
    and not stored when rows % 4 != 0): against float64 at 1e-5 (test_groupnorm_layernorm_add_pe's bound), nothing written behind the
    last row, and -- the promise beside layernorm256_kernel -- the same bits as layernorm_kernel on the same rows"""
    from s2d_amd import ops
    g = torch.Generator(device="cuda").manual_seed(rows * 2 + with_res)
    C = 256
    x = torch.randn((rows, C), device="cuda", generator=g) * 2 + 0.5
    r = torch.randn((rows, C), device="cuda", generator=g) if with_res else None
    ga = torch.randn((C,), device="cuda", generator=g) * 0.1 + 1
    be = torch.randn((C,), device="cuda", generator=g) * 0.1
    y = ops.layernorm(x, ga, be, res=r)
    inp = x.double() if r is None else x.double() + r.double()
    ref = torch.nn.functional.layer_norm(inp, (C,), ga.double(), be.double(), 1e-5)
    assert _rel64(y, ref) < 1e-5
    assert torch.equal(y, ops.layernorm(x, ga, be, res=r))
    # the same rows in pieces of at most 4095 rows go through layernorm_kernel
    parts = [ops.layernorm(x[s:s + 4095].contiguous(), ga, be, res=None if r is None else r[s:s + 4095].contiguous()) for s in range(0, rows, 4095)]
    assert torch.equal(torch.cat(parts), y)
    # into a larger buffer: the rows behind the last one keep their bits
    from s2d_amd._lib import lib
    wide = torch.full((rows + 16, C), 7.0, device="cuda")
    lib().call("s2d_layernorm_f32", x, r, ga, be, rows, C, 1e-5, wide, ops._stream())
    assert torch.equal(wide[:rows], y) and bool((wide[rows:] == 7.0).all())


@pytest.mark.parametrize("N,H,W,C", [(2, 17, 23, 64), (1, 1, 5, 8), (3, 32, 31, 64), (1, 33, 2, 12)])
def test_maxpool_odd_sizes_ties_and_argmax(N, H, W, C):
    """3 x 3 / stride 2 / pad 1 max pool at odd and even extents with many exact ties in a window (values drawn from 5 levels): values
    bit-equal to float64 max_pool2d of the same floats; want_idx returns the same values and a tap (ky * 3 + kx) that lies inside the map
    and holds the maximum"""
    from s2d_amd import ops
    g = torch.Generator(device="cuda").manual_seed(H * 100 + W)
    x = torch.randint(0, 5, (N, H, W, C), device="cuda", generator=g).float() - 2.0
    ref = torch.nn.functional.max_pool2d(x.double().permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1)
    y = ops.maxpool3x3s2(x)
    assert torch.equal(y.double(), ref)
    y2, idx = ops.maxpool3x3s2(x, want_idx=True)
    assert torch.equal(y2, y) and int(idx.max()) < 9
    Ho, Wo = y.shape[1:3]
    ky, kx = (idx // 3).long(), (idx % 3).long()
    yy = torch.arange(Ho, device="cuda")[None, :, None, None] * 2 - 1 + ky
    xx = torch.arange(Wo, device="cuda")[None, None, :, None] * 2 - 1 + kx
    assert bool(((yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)).all())
    n = torch.arange(N, device="cuda")[:, None, None, None].expand_as(idx)
    c = torch.arange(C, device="cuda")[None, None, None, :].expand_as(idx)
    assert torch.equal(x[n, yy, xx, c], y)
