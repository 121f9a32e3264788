"""The inputs and references of tests/test_gpu_attn_masks.py, checked without a GPU: the object-shaped masks really present whole
tiles and whole key splits masked (the regime random masks never reach), every special row has the property it is named for, the
bit packing round-trips and the reference agrees with a direct per-head loop."""
import math

import numpy as np
import pytest
import torch

from tests import attn_refs as R


@pytest.fixture(scope="module")
def masks_2760():
    return R.object_masks(2, 100, 3, 23, 40, torch.Generator().manual_seed(2760))


def test_splits_restates_the_launch_arithmetic():
    sp = R.splits(2760)
    assert (sp["tiles"], sp["S"], sp["tiles_per_split"], sp["nonempty"], sp["empty"]) == (87, 21, 5, 18, [18, 19, 20])
    assert (sp["bwd_S"], sp["bwd_tiles_per_split"], sp["bwd_scalar_tiles_per_split"]) == (11, 8, 4)
    assert len(sp["empty"]) >= 1 and 2760 % 32 != 0
    for K, S, tps in [(1, 1, 1), (31, 1, 1), (33, 1, 2), (129, 1, 5), (333, 2, 6), (1056, 8, 5), (20000, 32, 20)]:
        sp = R.splits(K)
        assert (sp["S"], sp["tiles_per_split"]) == (S, tps), K
        assert sp["nonempty"] * sp["tiles_per_split"] >= sp["tiles"] > (sp["nonempty"] - 1) * sp["tiles_per_split"]
    assert R.splits(20000)["bwd_S"] == 64 and R.splits(20000)["bwd_tiles_per_split"] == 10


def test_object_masks_present_whole_tiles_and_splits_masked(masks_2760):
    mask, info = masks_2760
    assert mask.shape == (2, 100, 2760) and info["K"] == 2760
    eff = R.effective(mask)
    tile, fwd, bwd = R.masked_shares(eff)
    print(f"wholly masked: (query, tile) {tile:.3f}  (query, forward split) {fwd:.3f}  (query, backward split) {bwd:.3f}")
    assert tile >= 0.5 and fwd >= 0.5 and bwd >= 0.5
    sp = R.splits(2760)
    first_free = (~eff).float().argmax(-1)                                  # every effective row has a free key
    late = int((first_free >= 2 * sp["tiles_per_split"] * R.KT).sum())
    print(f"queries whose first free key lies beyond the second forward split: {late}")
    assert late >= 20
    dead = eff[1].all(0)                                                     # keys of clip 1 masked for every query
    assert int(dead.sum()) >= 1
    hw = 23 * 40
    assert info["reserved_frame"] == 1 and bool(dead[hw:2 * hw].all())


def test_object_masks_special_rows(masks_2760):
    mask, info = masks_2760
    K, sp, hw = 2760, R.splits(2760), 23 * 40
    res = slice(info["reserved_frame"] * hw, (info["reserved_frame"] + 1) * hw)
    outside = torch.ones(K, dtype=torch.bool)
    outside[res] = False
    assert bool(mask[0, 0].all()) and not bool(mask[1, 0].all())
    for b in range(2):
        for qq, j in info["single"].items():
            free = (~mask[b, qq]).nonzero().flatten().tolist()
            assert free == [j], (b, qq, free)
        assert info["single"] == {1: 0, 2: K - 1, 3: 86 * 32}
        free4 = (~mask[b, 4]).nonzero().flatten()
        assert free4.tolist() == list(range(85 * 32, K)) and info["last_split_key"] == 17 * sp["tiles_per_split"] * 32
        assert (~mask[b, 5]).nonzero().flatten().tolist() == list(range(32))
        t = info["tile"]
        assert 0 < t < sp["tiles"] - 1 and t % sp["tiles_per_split"] not in (0, sp["tiles_per_split"] - 1)   # interior of a forward split too
        assert (~mask[b, 7]).nonzero().flatten().tolist() == list(range(32 * t, 32 * t + 32))
        keep = torch.ones(K, dtype=torch.bool) if b == 0 else outside
        assert not bool(mask[b, 6][keep].any())
        m8 = torch.zeros(K, dtype=torch.bool)
        m8[32 * t:32 * t + 32] = True
        assert torch.equal(mask[b, 8][keep], m8[keep])
    assert bool(mask[1, :, res].all())
    assert info["wave_clip"] == 0 and bool(mask[0, 32:64].all())
    assert not bool(mask[1].all(-1).any())                                   # clip 1: nobody attends everywhere by the all-masked rule
    assert not bool(mask[0, 31].all()) and not bool(mask[0, 64].all())       # the wave's neighbours keep their masks
    # ordinary rows: a box smaller than hl / 2 x wl / 3, the same in every frame it appears in
    for b, qq in [(0, 9), (0, 31), (0, 64), (1, 40), (1, 99)]:
        fr = (~mask[b, qq]).reshape(3, 23, 40)
        used = [t for t in range(3) if fr[t].any()]
        assert used and (b == 0 or 1 not in used)
        ys, xs = fr[used[0]].nonzero(as_tuple=True)
        h, w = int(ys.max() - ys.min()) + 1, int(xs.max() - xs.min()) + 1
        assert h < 23 / 2 and w < 40 / 3 and int(fr[used[0]].sum()) == h * w
        for t in used[1:]:
            assert torch.equal(fr[t], fr[used[0]])


@pytest.mark.parametrize("B,Q,T,hl,wl", [(2, 37, 1, 9, 37), (2, 128, 2, 16, 33), (1, 100, 3, 23, 40)])
def test_object_masks_other_shapes(B, Q, T, hl, wl):
    mask, info = R.object_masks(B, Q, T, hl, wl, torch.Generator().manual_seed(T * hl * wl))
    K = T * hl * wl
    eff = R.effective(mask)
    tile, fwd, bwd = R.masked_shares(eff)
    print(f"K={K} Q={Q}: wholly masked (query, tile) {tile:.3f} forward split {fwd:.3f} backward split {bwd:.3f}")
    assert tile >= 0.5
    assert info["reserved_frame"] is None and bool(mask[0, 0].all())
    assert (info["wave_clip"] is None) == (Q < 64)
    if Q >= 64:
        assert bool(mask[info["wave_clip"], 32:64].all())
    for qq, j in info["single"].items():
        assert (~mask[-1, qq]).nonzero().flatten().tolist() == [j]
    assert not bool(mask[:, 6].any())
    assert (K % 32 == 0) == (K == 1056)


@pytest.mark.parametrize("Q", [1, 31, 32, 33, 100, 128])
def test_pack_bits_round_trips(Q):
    g = torch.Generator().manual_seed(Q)
    mask = torch.rand((2, Q, 77), generator=g) < 0.5
    mask[0, 0] = True
    mask[1, Q - 1] = True
    bits, unm = R.pack_bits(mask)
    assert bits.shape == (2, 77, 4) and bits.dtype == torch.int32 and unm.shape == (2, 4) and unm.dtype == torch.int32
    back, free = R.unpack_bits(bits, unm, Q)
    assert torch.equal(back, mask)
    assert torch.equal(free, ~mask.all(-1))
    # bit by bit, and nothing set for queries >= Q
    w = bits.numpy().view(np.uint32)
    for qq in range(128):
        col = (w[:, :, qq // 32] >> (qq % 32)) & 1
        if qq < Q:
            np.testing.assert_array_equal(col.astype(bool), mask[:, qq].numpy())
        else:
            assert not col.any()
    u = unm.numpy().view(np.uint32)
    for qq in range(Q, 128):
        assert not ((u[:, qq // 32] >> (qq % 32)) & 1).any()


def _loop_ref(q, k, v, mask, H):
    """direct per-head float64 loop (numpy), all-masked rows reset by hand; -> out, lse2"""
    B, Q, C = q.shape
    d = C // H
    out, lse = np.zeros((B, Q, C)), np.zeros((B, H, Q))
    for b in range(B):
        for h in range(H):
            s = (q[b, :, h * d:(h + 1) * d] / math.sqrt(d)) @ k[b, :, h * d:(h + 1) * d].T
            if mask is not None:
                m = mask[b].copy()
                m[m.all(-1)] = False
                s = np.where(m, -np.inf, s)
            top = s.max(-1, keepdims=True)
            a = np.exp(s - top)
            lse[b, h] = (top[:, 0] + np.log(a.sum(-1))) / math.log(2.0)
            out[b, :, h * d:(h + 1) * d] = (a / a.sum(-1, keepdims=True)) @ v[b, :, h * d:(h + 1) * d]
    return out, lse


def test_masked_attn_ref_agrees_with_a_per_head_loop():
    g = torch.Generator().manual_seed(11)
    B, Q, K, C, H = 2, 37, 333, 64, 2
    q, k, v, dout = (torch.randn(s, generator=g, dtype=torch.float64) for s in [(B, Q, C), (B, K, C), (B, K, C), (B, Q, C)])
    mask, _ = R.object_masks(B, Q, 1, 9, 37, torch.Generator().manual_seed(3))
    for m in (mask, None):
        out, lse, dq, dk, dv = R.masked_attn_ref(q, k, v, m, H, torch.float64, dout)
        o2, l2 = R.masked_attn_ref(q, k, v, m, H, torch.float64)
        assert torch.equal(o2, out) and torch.equal(l2, lse)
        ro, rl = _loop_ref(q.numpy(), k.numpy(), v.numpy(), None if m is None else m.numpy(), H)
        np.testing.assert_allclose(out.numpy(), ro, rtol=0, atol=1e-13 * np.abs(ro).max())
        np.testing.assert_allclose(lse.numpy(), rl, rtol=0, atol=1e-13 * np.abs(rl).max())
        # gradients: central differences of sum(out * dout) along random directions
        for t, gr in ((q, dq), (k, dk), (v, dv)):
            u = torch.randn(t.shape, generator=g, dtype=torch.float64)
            eps = 1e-6
            args = {"q": q, "k": k, "v": v}
            name = "q" if t is q else ("k" if t is k else "v")
            f = lambda x: float((R.masked_attn_ref(**{**args, name: x}, mask=m, H=H, dtype=torch.float64)[0] * dout).sum())
            num = (f(t + eps * u) - f(t - eps * u)) / (2 * eps)
            assert abs(num - float((gr * u).sum())) < 1e-6 * max(1.0, abs(num)), (name, num, float((gr * u).sum()))
    # exact zeros where no query attends, and a float32 evaluation close to the float64 one
    mask = mask.clone()
    mask[1, :, 40:50] = True
    mask[1, 6] = mask[1, 9]                     # nobody in clip 1 attends everywhere
    eff = R.effective(mask)
    out, lse, dq, dk, dv = R.masked_attn_ref(q, k, v, mask, H, torch.float64, dout)
    dead = eff.all(1)
    assert bool(dead.any()) and not bool(dk[dead].any()) and not bool(dv[dead].any())
    o32 = R.masked_attn_ref(q.float(), k.float(), v.float(), mask, H, torch.float32)[0]
    assert o32.dtype == torch.float32 and float((o32.double() - out).abs().max()) < 1e-5 * float(out.abs().max())
    # a single free key: the output row is that value row and the query gradient vanishes
    j = 0
    assert torch.allclose(out[:, 1], v[:, j], rtol=0, atol=1e-14) and float(dq[:, 1].abs().max()) < 1e-14
