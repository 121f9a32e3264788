"""Data-path and optimizer kernels around the training step (csrc/augment.hip, csrc/optim.hip) against exact references at the sizes
`python -m s2d_amd.train` runs them at: the float64 references, the inputs and the band rule of tests/test_data_refs_cpu.py (which
proves, without a GPU, that the float32 mirror of the oracle and CPU torch stay inside the same rule on the same inputs), and
`reference_step` of tests/test_gpu_optim.py.  Every case is the smallest shape that reaches the code it names:

  frames      720 x 1280 -> short edge 360 under brightness + contrast + rotation + crop + flip (W1 = 438: a second x-block with dead
              lanes), and without crop to 203 x 361 (W1 % 4 != 0); CHW and HWC, bit-identical, cmean written back exactly.
  masks       480 x 854 (W0 % 32 != 0) and 720 x 1280 bit planes and u8 planes, T x S = 2 x 4 with dummy slots, odd output planes so
              later planes start off a word; the two kernels bit-identical, area = plane sums.
  paste       s2d_copy_paste_frame_u8 at 720 x 1278 (five x-blocks: full waves, and a last block with two dead lanes),
              K up to 64 (bit 63 of the lane's copy set), two consecutive frames (the second resizes the first's canvas); the integer
              tables against counts taken from the device's own canvas.  s2d_copy_paste_u8 / s2d_copy_paste_overlap, which nothing in
              s2d_amd calls, through the C ABI.  Sources and outputs are views into larger buffers with poisoned guards: a read
              past a plane's last row shows up as a set pixel, a write past an output as a changed guard byte.
  shift       s2d_shift_planes_u8 in propagate_sparse_masks' plan format: the 16-byte tail, unaligned and unshifted planes, every
              (dx, dy) of {0, +-1, +-2}^2, the second trip of the grid-stride loop, and u8 sources holding values other than 0 / 1
              (the vector path used to copy them through; include/s2d_hip.h says `!= 0`).
  optimizer   more than 256 chunks (the finalize loop wraps), a 5 * 16384 + 3 tensor, a multi-chunk tensor without gradient, a
              parameter and a teacher one float into their storage (the scalar path).

Lines starting `datarow` carry the figures profiles/data_path_parity.txt records."""
import numpy as np
import pytest
import torch

from tests import test_data_refs_cpu as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 8192


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)


def _guarded(shape, fill, data=None, offset=0):
    """-> (view of `shape` starting `offset` bytes into a u8 buffer filled with `fill`, the buffer); data (host u8) is copied in"""
    n = int(np.prod(shape))
    buf = torch.full((offset + n + GUARD,), fill, device=DEV, dtype=torch.uint8)
    view = buf[offset:offset + n].view(*shape)
    if data is not None:
        view.copy_(_dev(data))
    return view, buf


def _guard_intact(buf, n, fill, offset=0):
    return bool((buf[:offset] == fill).all()) and bool((buf[offset + n:] == fill).all())


# --------------------------------------------------------------------------- clip augmentation
@pytest.mark.parametrize("name", list(R.FRAME_CASES))
def test_warp_frames_vs_float64(name):
    from s2d_amd._lib import lib
    from s2d_amd.data.augment import augment_frames_hwc
    fr, P, hw, ref, band, excl = R.frame_case(name)
    T, _, H0, W0 = fr.shape
    H1, W1 = hw
    x = _dev(fr)
    p_chw, p_hwc = _dev(P), _dev(P)
    got, gbuf = _guarded((T, 3, H1, W1), 7)
    lib().call("s2d_aug_warp_frames_u8", x, T, H0, W0, p_chw, H1, W1, got, _stream())
    hwc = augment_frames_hwc(x.permute(0, 2, 3, 1).contiguous(), p_hwc, hw)
    torch.cuda.synchronize()
    assert _guard_intact(gbuf, got.numel(), 7)
    R.check_levels(f"kernel frames {name}", got.cpu().numpy(), ref, band, excl)
    assert torch.equal(hwc, got)                                          # HWC == CHW, bit for bit
    assert torch.equal(p_hwc, p_chw)                                      # same cmean bits, the scratch words back to 0
    back = p_chw.cpu().numpy()
    for t in range(T):
        want = R.crop_mean_f64(fr[t], P[t])[1]
        assert back[t, 12].tobytes() == want.tobytes(), (t, back[t, 12], want)
    keep = [i for i in range(16) if i != 12]
    np.testing.assert_array_equal(back[:, keep], P[:, keep])


@pytest.mark.parametrize("name", list(R.MASK_CASES))
def test_warp_masks_and_bit_planes_vs_float64(name):
    from s2d_amd import ops
    from s2d_amd._lib import lib
    from s2d_amd.data.augment import warp_mask_bits
    planes, plane_of, u8, P, hw, ref, amb = R.mask_case(name)
    S, T, H0, W0 = u8.shape
    H1, W1 = hw
    p = _dev(P)
    mo, mbuf = _guarded((S, T, H1, W1), 7)
    lib().call("s2d_aug_warp_masks_u8", _dev(u8), S, T, H0, W0, p, H1, W1, mo, _stream())
    bits = ops.pack_mask_bits(_dev(planes).view(planes.shape[0], -1).contiguous())
    out, area = warp_mask_bits(bits, plane_of, H0, W0, p, hw)
    torch.cuda.synchronize()
    assert _guard_intact(mbuf, mo.numel(), 7)
    R.check_exact(f"kernel masks {name}", mo.cpu().numpy(), ref, amb)
    assert int(mo.max()) == 1
    assert torch.equal(out, mo.permute(1, 0, 2, 3))                       # the two kernels agree bit for bit
    assert area.cpu().tolist() == out.view(T, S, -1).sum(-1, dtype=torch.int64).cpu().tolist()
    assert int(area[0, 1]) == 0 and int(area[1, 2]) == 0 and int((area > 0).sum()) == 6


# --------------------------------------------------------------------------- video copy-paste
def _counts(canvas, tm):
    """canvas bool [K,H,W], tm bool [N,H,W] (device) -> (inter [K,N], tarea [N], alive [N]) as python lists"""
    alpha = canvas.any(0)
    inter = [[int((c & m).sum()) for m in tm] for c in canvas]
    return inter, [int(m.sum()) for m in tm], [int((m & ~alpha).sum()) for m in tm]


@pytest.mark.parametrize("K,N", R.PASTE_KN)
def test_copy_paste_frame_vs_float64_and_torch(K, N):
    from s2d_amd._lib import lib
    sf, sm, tf, tm = R.paste_inputs(K, N)
    H, W, Hs, Ws = R.PASTE_H, R.PASTE_W, R.PASTE_HS, R.PASTE_WS
    assert W % 256 != 0 and W % 64 != 0
    sfd, _ = _guarded((3, Hs, Ws), 255, sf)
    cur, _ = _guarded((K, Hs, Ws), 1, sm)
    cur_host = sm
    for f, geo in enumerate(R.PASTE_GEO):
        canvas, cbuf = _guarded((K, H, W), 1)                             # its guard is the next frame's source guard: poison 1
        of, obuf = _guarded((3, H, W), 7)
        ot, tbuf = _guarded((max(N, 1), H, W), 7)
        st = torch.full((K * N + 2 * N + 1,), -12345, device=DEV, dtype=torch.int32)       # the call zeroes its tables
        tmd = _dev(tm[f]) if N else torch.zeros((1,), device=DEV, dtype=torch.uint8)
        lib().call("s2d_copy_paste_frame_u8", sfd, Hs, Ws, cur, K, cur.shape[1], cur.shape[2], _dev(tf[f]), tmd, N, H, W, *geo, canvas, of,
                   ot, st, st[K * N:], st[K * N + N:], _stream())
        torch.cuda.synchronize()
        assert _guard_intact(cbuf, canvas.numel(), 1) and _guard_intact(obuf, of.numel(), 7)
        assert _guard_intact(tbuf, N * H * W, 7) and int(st[-1]) == -12345
        got = dict(canvas=canvas.cpu().numpy(), frame=of.cpu().numpy(), tgt=ot[:N].cpu().numpy())
        ref = R.paste_frame_f64(sf, cur_host, tf[f], tm[f], geo)
        assert ref["canvas"][K - 1].any() and ref["canvas"][0].any() and int(got["canvas"].max()) == 1
        R.check_paste(f"kernel paste K={K} N={N} frame {f}", got, ref)
        # torch's own float32 calls: wherever the float64 value is outside the band, the three agree
        tor = R.paste_frame_torch(sf, cur_host, tf[f], tm[f], geo)
        R.check_exact(f"kernel paste K={K} N={N} frame {f} canvas vs torch", got["canvas"], tor["canvas"], ref["amb"])
        R.check_levels(f"kernel paste K={K} N={N} frame {f} composite vs torch", got["frame"], tor["frame"], ref["frame_band"],
                       (ref["alpha_amb"] | (tor["alpha"] != ref["alpha"]))[None])
        if N:
            tab = st.cpu().numpy()
            inter, tarea, alive = tab[:K * N].reshape(K, N), tab[K * N:K * N + N], tab[K * N + N:K * N + 2 * N]
            # the ballots must not lose a lane: exactly the counts of the device's own canvas
            ci, ca, cl = _counts(canvas.bool(), tmd.bool())
            assert inter.tolist() == ci and tarea.tolist() == ca and alive.tolist() == cl
            # and the reference's, up to the ambiguous pixels (none on these inputs unless the figures above say otherwise)
            tmb = tm[f] != 0
            slack_i = np.array([[int((ref["amb"][k] & tmb[n]).sum()) for n in range(N)] for k in range(K)])
            slack_a = np.array([int((ref["alpha_amb"] & tmb[n]).sum()) for n in range(N)])
            assert (np.abs(inter - ref["inter"]) <= slack_i).all() and (np.abs(alive - ref["alive"]) <= slack_a).all()
            np.testing.assert_array_equal(tarea, ref["tarea"])
            assert tarea[0] >= H + 2 * W - 3 and inter.any() and (alive < tarea).any()
            print(f"datarow kernel paste K={K} N={N} frame {f} tables: equal to the counts of the device canvas; slack against the reference "
                  f"inter {int(slack_i.sum())} alive {int(slack_a.sum())} pixels, max |inter - ref| {int(np.abs(inter - ref['inter']).max())}")
        cur, cur_host = canvas, got["canvas"]                             # the next frame resizes this canvas


def test_copy_paste_clip_and_overlap_through_the_abi():
    """s2d_copy_paste_u8 and s2d_copy_paste_overlap (exported, called by nothing in s2d_amd): T = 2, 200 x 300, K = 3, N = 2, keep[1] = 0"""
    from s2d_amd._lib import lib
    sf, sm, tf, tm = R.clip_inputs()
    K, N, T, (H, W), (Hs, Ws) = 3, 2, 2, tf.shape[2:], sf.shape[1:]
    sfd, _ = _guarded((3, Hs, Ws), 255, sf)
    smd, _ = _guarded((K, Hs, Ws), 1, sm)
    of, obuf = _guarded((T, 3, H, W), 7)
    om, mbuf = _guarded((N + K, T, H, W), 7)
    geo = _dev(np.array(R.CLIP_GEO, np.int32))
    keep = _dev(np.array(R.CLIP_KEEP, np.uint8))
    tmd = _dev(tm)
    lib().call("s2d_copy_paste_u8", _dev(tf), tmd, N, T, H, W, sfd, smd, K, Hs, Ws, geo, keep, of, om, _stream())
    tab = torch.full((K * N + N + 1,), -12345, device=DEV, dtype=torch.int32)
    lib().call("s2d_copy_paste_overlap", tmd, N, T, H, W, smd, K, Hs, Ws, *R.CLIP_GEO[0], tab, tab[K * N:], _stream())
    torch.cuda.synchronize()
    assert _guard_intact(obuf, of.numel(), 7) and _guard_intact(mbuf, om.numel(), 7) and int(tab[-1]) == -12345
    kept = np.array(R.CLIP_KEEP, bool)
    frames, masks = of.cpu().numpy(), om.cpu().numpy()
    assert int(masks.max()) == 1 and not masks[N + 1].any() and masks[N].any() and masks[N + 2].any()
    for t in range(T):
        ref = R.paste_frame_f64(sf, sm, tf[t], tm[:, t], R.CLIP_GEO[t], keep=R.CLIP_KEEP)
        want = dict(ref, canvas=ref["canvas"] * kept[:, None, None].astype(np.uint8), amb=ref["amb"] & kept[:, None, None])
        R.check_paste(f"kernel clip frame {t}", dict(canvas=masks[N:, t], frame=frames[t], tgt=masks[:N, t]), want)
        if t == 0:                                                        # the overlap call sees every copy, kept or not
            counts, area = tab[:K * N].view(K, N).cpu().numpy(), tab[K * N:K * N + N].cpu().numpy()
            tmb = tm[:, 0] != 0
            slack = np.array([[int((ref["amb"][k] & tmb[n]).sum()) for n in range(N)] for k in range(K)])
            assert (np.abs(counts - ref["inter"]) <= slack).all() and counts.any()
            np.testing.assert_array_equal(area, ref["tarea"])
            print(f"datarow kernel overlap: max |counts - ref| {int(np.abs(counts - ref['inter']).max())}, slack {int(slack.sum())} pixels")


# --------------------------------------------------------------------------- sparse-mask densification
def _shift(rows, H, W):
    """rows: [(source plane tensor [H,W] on the device, dx, dy)] in propagate_sparse_masks' plan format -> u8 [n,H,W] (host)"""
    from s2d_amd._lib import lib
    table = np.zeros((len(rows),), dtype=[("src", np.uint64), ("dx", np.int32), ("dy", np.int32)])
    table["src"], table["dx"], table["dy"] = zip(*[(p.data_ptr(), dx, dy) for p, dx, dy in rows])
    plan = torch.from_numpy(table.view(np.int64).reshape(-1, 2)).to(DEV)
    out, buf = _guarded((len(rows), H, W), 7)
    lib().call("s2d_shift_planes_u8", plan, len(rows), H, W, out, _stream())
    torch.cuda.synchronize()
    assert _guard_intact(buf, out.numel(), 7)
    return out.cpu().numpy()


def _sources(H, W, seed):
    """four source planes on the device: u8 holding 0 / 1 / 255 at a 16-aligned address, u8 one byte into its buffer, bool aligned,
    bool three bytes into its buffer -> [(tensor, host array)]"""
    rng = np.random.default_rng(seed)
    out = []
    for dtype, offset in ((np.uint8, 0), (np.uint8, 1), (bool, 0), (bool, 3)):
        host = rng.choice(np.array([0, 0, 1, 255], np.uint8), size=(H, W))
        if dtype is bool:
            host = host != 0
        view, _ = _guarded((H, W), 9, host.view(np.uint8), offset)
        assert view.data_ptr() % 16 == offset
        out.append((view if dtype is np.uint8 else view.view(torch.bool), host))
    return out


def test_shift_planes_tail_unaligned_and_every_shift():
    """37 x 53 (H * W % 16 != 0: every plane ends in a partial 16-byte group and all output planes but the first start unaligned)"""
    H, W = 37, 53
    src = _sources(H, W, 0)
    rows, planes, shifts = [], [], []
    for i, (dx, dy) in enumerate([(0, 0)] * 4 + [(dx, dy) for dy in (0, 1, -1, 2, -2) for dx in (0, 1, -1, 2, -2)]):
        t, h = src[i % 4]                                                 # the first four: each source unshifted; row 0 takes the vector path
        rows.append((t, dx, dy)); planes.append(h); shifts.append((dx, dy))
    assert {(0, 2), (0, -2), (2, 0), (-2, -2)} <= set(shifts)
    got = _shift(rows, H, W)
    want = R.shift_planes_np(planes, shifts)
    np.testing.assert_array_equal(got, want)
    assert got.max() == 1 and all(w.any() for w in want)


def test_shift_planes_u8_source_values_become_0_or_1():
    """the header's contract `out = src != 0` for a u8 source holding 0 / 1 / 255 on the 16-byte vector path (aligned, unshifted, a
    whole number of groups) as on the byte path"""
    H, W = 64, 80
    src = _sources(H, W, 1)
    assert src[0][1].max() == 255
    got = _shift([(src[0][0], 0, 0), (src[0][0], 1, 0), (src[1][0], 0, 0)], H, W)
    assert got.max() == 1
    np.testing.assert_array_equal(got, R.shift_planes_np([src[0][1], src[0][1], src[1][1]], [(0, 0), (1, 0), (0, 0)]))


def test_shift_planes_second_trip_of_the_grid_stride_loop():
    """2050 x 2048 = 4 198 400 > 1024 blocks x 4096 bytes: the last 4096 bytes of every plane are a second trip"""
    H, W = 2050, 2048
    assert H * W > 1024 * 4096
    src = _sources(H, W, 2)
    rows = [(src[0][0], 0, 0), (src[3][0], 1, -2), (src[1][0], 0, 0)]
    got = _shift(rows, H, W)
    want = R.shift_planes_np([src[0][1], src[3][1], src[1][1]], [(0, 0), (1, -2), (0, 0)])
    np.testing.assert_array_equal(got, want)
    assert want[:, -2:].any()


# --------------------------------------------------------------------------- optimizer
def test_optimizer_many_chunks_odd_tail_none_grad_and_unaligned_storage():
    from s2d_amd.optim import CHUNK, FullModelGradientClippingAdamW
    from tests.test_gpu_optim import reference_step
    clip, inv_scale, m = 0.01, 1.0 / 1024, 0.999
    rng = np.random.default_rng(0)
    shapes = [(int(n),) for n in rng.integers(1, 700, 296)] + [(5 * CHUNK + 3,), (2 * CHUNK + 1,), (40001,), (2 * CHUNK,)]
    I_TAIL, I_NONE, I_VIEW = 296, 297, 298
    g = torch.Generator().manual_seed(3)
    init = [torch.randn(s, generator=g) * 0.1 for s in shapes]
    ref_p = [torch.nn.Parameter(x.clone()) for x in init]
    ref_t = [x.clone() + 0.01 for x in init]
    groups = [{"params": [p], "lr": 1e-4 * (1 + (i % 3)), "weight_decay": [0.05, 0.0, 0.01][i % 3]} for i, p in enumerate(ref_p)]
    ref_opt = torch.optim.AdamW(groups, 1e-4)

    def on_dev(x, off):                                                   # off floats into its own storage
        store = torch.zeros((x.numel() + off,), device=DEV)
        store[off:].copy_(x)
        return store[off:].view(x.shape)
    hip_p = [torch.nn.Parameter(on_dev(x, 1 if i == I_VIEW else 0)) for i, x in enumerate(init)]
    hip_t = [on_dev(x + 0.01, 1 if i in (I_VIEW, I_TAIL) else 0) for i, x in enumerate(init)]
    assert hip_p[I_VIEW].data_ptr() % 16 == 4 and hip_t[I_TAIL].data_ptr() % 16 == 4 and hip_p[I_TAIL].data_ptr() % 16 == 0
    hgroups = [{"params": [p], "lr": gr["lr"], "weight_decay": gr["weight_decay"]} for p, gr in zip(hip_p, groups)]
    opt = FullModelGradientClippingAdamW(hgroups, lr=1e-4, clip_norm=clip, ema_params=hip_t)       # ops._chk accepts the offset views
    assert len(shapes) >= 300 and opt._nchunks > 256 + 8
    for step in range(3):
        gs = torch.Generator().manual_seed(20 + step)
        grads = [torch.randn(s, generator=gs) * 0.1 / inv_scale for s in shapes]
        grads[I_NONE] = None
        reference_step(ref_p, ref_t, grads, ref_opt, clip, inv_scale, m)
        opt.zero_grad()
        for p, gr in zip(hip_p, grads):
            if gr is not None:
                p.grad.copy_(gr.to(DEV))
        hip_p[I_NONE].grad.fill_(float("nan"))                            # must not be read: torch skips a parameter without gradient
        opt._t_ptrs[5 * I_NONE + 1] = 0
        opt.step(inv_scale=inv_scale, ema_momentum=m)
        tot = torch.sqrt(sum((gr.double() * inv_scale).pow(2).sum() for gr in grads if gr is not None))
        assert float(tot) > clip                                          # the clip is on
        np.testing.assert_allclose(opt.grad_norm(), float(tot), rtol=1e-6)
        assert not opt.found_inf()
        for i, (a, b) in enumerate(zip(hip_p, ref_p)):
            np.testing.assert_allclose(a.detach().cpu().numpy(), b.detach().numpy(), rtol=2e-6, atol=1e-8, err_msg=f"param {i} step {step}")
        for i, (a, b) in enumerate(zip(hip_t, ref_t)):
            np.testing.assert_allclose(a.cpu().numpy(), b.numpy(), rtol=2e-6, atol=1e-8, err_msg=f"teacher {i} step {step}")
    np.testing.assert_array_equal(hip_p[I_NONE].detach().cpu().numpy(), init[I_NONE].numpy())      # no decay, no update
    sd, rsd = opt.state_dict(), ref_opt.state_dict()
    assert I_NONE not in rsd["state"] and float(sd["state"][I_NONE]["exp_avg"].abs().max()) == 0.0
    for i in rsd["state"]:
        for key in ("exp_avg", "exp_avg_sq"):
            want = rsd["state"][i][key].numpy()
            np.testing.assert_allclose(sd["state"][i][key].cpu().numpy(), want, rtol=2e-6, atol=4e-7 * np.abs(want).max(), err_msg=f"{key} {i}")
        assert float(sd["state"][i]["step"]) == float(rsd["state"][i]["step"])
