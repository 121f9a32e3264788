"""The point loss (csrc/loss.hip) on exact inputs: the tie rule of the top-k selection -- ascending |logit|, then ascending point
index; the reference's torch.topk leaves ties open -- on every path that breaks ties (list / block scan, one / two map parts, injected /
generated points, streamed / recomputed rows, more than 4096 rows in one call), and the int32 fixed-point gradient scatter under
clustered points.  tests/point_loss_refs.py builds the cases and the float64 reference; tests/test_point_loss_refs_cpu.py shows that
the keys tie identically in fp32 and float64 and that the reversed rule would miss the bars used here by a factor of 100 or more.

Bars: losses rtol 1e-5 (the op-level summation-order bar of tests/test_gpu_c4_oracle.py), gradients max-norm relative 2e-5
(tests/test_gpu_backward.py).  One `ptrow <case> <loss|grad> <figure>` line per comparison."""
import functools

import numpy as np
import pytest
import torch

from tests import point_loss_refs as R

pytestmark = pytest.mark.gpu
W_MASK, W_DICE = 5.0, 5.0


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _forward(op, P, keep=False, coords=True, **kw):
    from s2d_amd import ops
    tgt, cnt = _dev(op["tgt"]), _dev(op["cnt"])
    ne = ops.target_nonempty(tgt, cnt)
    assert bool(ne.all())                                            # every (target, frame) plane non-empty: every matched row active
    if coords:
        kw.update(coords_over=_dev(op["cov"]), coords_rand=_dev(op["crd"]))
    return ops.point_loss(_dev(op["ml"]), tgt, cnt, ne, _dev(op["iq"]), _dev(op["it"]), _dev(op["nm"]), op["dims"], P, keep=keep, **kw)


@functools.lru_cache(maxsize=None)
def _case(name):
    c = R.exact_case(name)
    R.check_structure(c)
    return c, R.loss_masks_ref(c["src"], c["tt"], c["cov"], c["crd"], c["n_unc"], c["num_masks"], W_MASK, W_DICE)


def _check_losses(tag, L, ref):
    L = np.asarray(L, np.float64).reshape(-1, 2)
    err = max(abs(L[:, 0] - ref[0]).max() / abs(ref[0]), abs(L[:, 1] - ref[1]).max() / abs(ref[1]))
    print(f"ptrow {tag} loss {err:.3e}")
    np.testing.assert_allclose(L[:, 0], ref[0], rtol=R.LOSS_RTOL, err_msg=tag)
    np.testing.assert_allclose(L[:, 1], ref[1], rtol=R.LOSS_RTOL, err_msg=tag)


def _check_grad(tag, g, want):
    err = R.rel(g, want)
    print(f"ptrow {tag} grad {err:.3e}")
    assert err < R.GRAD_REL, (tag, err)


# A (list path), B (block scan), C (two map parts: the backward's per-tie ownership test)
@pytest.mark.parametrize("name", [n for n in R.CASES if not n.startswith("E_")])
def test_streamed_rows_keep_the_lowest_index_ties(name):
    from s2d_amd import ops
    c, ref = _case(name)
    op = R.op_inputs(c)
    L, ctx = _forward(op, c["P"], keep=True)
    g = ops.point_loss_backward(ctx, W_MASK, W_DICE)
    assert ops.point_loss_kept_rows(ctx) == ([4], 4)
    _check_losses(name, L.cpu().numpy(), ref)
    _check_grad(name, g.cpu().numpy().reshape(ref[2].shape), ref[2])
    L2, ctx2 = _forward(op, c["P"], keep=True)
    assert torch.equal(L, L2) and torch.equal(g, ops.point_loss_backward(ctx2, W_MASK, W_DICE))


# D: generator mode on a map of two parts with a zero plateau: more exact-zero keys than n_unc, in both parts' index ranges.  P = 2048:
# streamed rows, forward and backward (tie_before); P = 2050 (3P not a multiple of 4): recomputed rows, forward
@pytest.mark.parametrize("P", [2048, 2050])
def test_generated_points_spend_ties_across_index_ranges(P):
    from s2d_amd import ops
    from s2d_amd._lib import lib
    hm, wm, H, W, S = 128, 256, 256, 512, 20251
    streamed = (3 * P) % 4 == 0
    rng = np.random.default_rng(41)
    src = rng.choice(np.array((1, 2, 3), np.float32), (4, hm, wm))        # positive above the plateau: no key but the plateau's is 0
    src[:, 40:] = 0
    c = dict(src=src, tt=R.block_targets(rng, 4, H, W), cov=np.zeros((4, 3 * P, 2), np.float32), crd=np.zeros((4, 0, 2), np.float32),
             map=(hm, wm), tgt=(H, W), vals=(1, 2, 3), seed=41)
    op = R.op_inputs(c)
    uv = torch.empty((4, 3 * P, 2), device="cuda", dtype=torch.float32)
    bounds = torch.zeros((4, 9), device="cuda", dtype=torch.int32)
    scratch = torch.empty((5,), device="cuda", dtype=torch.int32)
    lib().call("s2d_point_loss_rng_points", S, hm, wm, 0, 4, 3 * P, uv, bounds, scratch, torch.cuda.current_stream().cuda_stream)
    cov, bh = uv.cpu().numpy(), bounds.cpu().numpy()
    zero = R.sample_np(src, cov, np.float32) == 0
    for r in range(4):
        assert bh[r, 0] == 0 and bh[r, 2] == 3 * P and 0 < bh[r, 1] < 3 * P
        n0, n1 = int(zero[r, :bh[r, 1]].sum()), int(zero[r, bh[r, 1]:].sum())
        assert n0 + n1 > P and n0 > 0 and n1 > 0, (r, n0, n1)              # n_unc = P at importance 1: threshold key 0, ties in both ranges
    tag = f"D_p{P}"
    La, ca = _forward(op, P, keep=True, coords=False, importance=1.0, seed=S)
    Lb, cb = _forward(dict(op, cov=cov[None], crd=c["crd"][None]), P, keep=True, importance=1.0)
    print(f"ptrow {tag}_generated_vs_injected loss {float(((La - Lb).abs() / Lb.abs()).max()):.3e}")
    np.testing.assert_allclose(La.cpu().numpy(), Lb.cpu().numpy(), rtol=2e-6)
    La2, ca2 = _forward(op, P, keep=True, coords=False, importance=1.0, seed=S)
    assert torch.equal(La, La2)
    ref = R.loss_masks_ref(src, c["tt"], cov, c["crd"], P, 2.0, W_MASK, W_DICE)
    _check_losses(f"{tag}_injected", Lb.cpu().numpy(), ref)
    if streamed:
        ga, gb = ops.point_loss_backward(ca, W_MASK, W_DICE), ops.point_loss_backward(cb, W_MASK, W_DICE)
        print(f"ptrow {tag}_generated_vs_injected grad {float((ga - gb).abs().max() / gb.abs().max()):.3e}")
        assert float(ga.abs().max()) > 0
        assert float((ga - gb).abs().max()) <= 4e-6 * float(gb.abs().max())
        assert torch.equal(ga, ops.point_loss_backward(ca2, W_MASK, W_DICE))
        _check_grad(f"{tag}_injected", gb.cpu().numpy().reshape(ref[2].shape), ref[2])


# E: rows whose samples are not kept (3P or P/4 not a multiple of 4, H*W not a multiple of 32): the recompute kernels, forward only
@pytest.mark.parametrize("name", [n for n in R.CASES if n.startswith("E_")])
def test_recomputed_rows_keep_the_lowest_index_ties(name):
    c, ref = _case(name)
    op = R.op_inputs(c)
    L = _forward(op, c["P"])
    L2 = _forward(op, c["P"])
    print(f"ptrow {name} two runs {L.cpu().numpy().ravel().tolist()} {L2.cpu().numpy().ravel().tolist()}")
    _check_losses(name, L.cpu().numpy(), ref)
    assert torch.equal(L, L2)


# F: 5120 active rows in one call: the first 4096 streamed, the last 1024 (layers 8 and 9) recomputed by the same launches
@pytest.mark.parametrize("kind", ["smooth", "ties"])
def test_more_than_4096_rows_in_one_call(kind):
    from s2d_amd import ops
    c = R.many_rows_case(kind)
    ref = R.loss_masks_ref(c["src"], c["tt"], c["cov"], c["crd"], c["n_unc"], c["num_masks"])
    L, ctx = _forward(c["op"], c["P"], keep=True)
    assert ops.point_loss_kept_rows(ctx) == ([512] * 10, 5120)
    Lh = L.cpu().numpy()
    print(f"ptrow F_{kind} layers {Lh[:, 0].tolist()} {Lh[:, 1].tolist()}")
    _check_losses(f"F_{kind}_streamed_layers", Lh[:8], ref)
    _check_losses(f"F_{kind}_recomputed_layers", Lh[8:], ref)
    assert torch.equal(L, _forward(c["op"], c["P"]))
    with pytest.raises(NotImplementedError):
        ops.point_loss_backward(ctx, W_MASK, W_DICE)


# G: every point of a row on one pixel / one four-tap corner / one 2 x 2 block: the int32 gradient tile must not wrap, and its row scale
# is a power of two, so a power-of-two multiple of the weights gives the same integer sums
@pytest.mark.parametrize("placement", R.G_PLACEMENTS)
def test_gradient_scatter_under_clustered_points(placement):
    from s2d_amd import ops
    c = R.cluster_case(placement)
    args = (c["src"], c["tt"], c["cov"], c["crd"], c["n_unc"], c["num_masks"])
    lm, ld, g_mask = R.loss_masks_ref(*args, 1.0, 0.0)
    g_dice = R.loss_masks_ref(*args, 0.0, 1.0)[2]
    L, ctx = _forward(R.op_inputs(c), c["P"], keep=True)
    _check_losses(c["name"], L.cpu().numpy(), (lm, ld))
    got = {}
    for k, (wm_, wd_) in enumerate(R.G_WEIGHTS):
        got[k] = ops.point_loss_backward(ctx, wm_, wd_)
        g, want = got[k].cpu().numpy().reshape(g_mask.shape), wm_ * g_mask + wd_ * g_dice
        _check_grad(f"{c['name']}_w{k}", g, want)
        for r in range(4):                                            # the hot pixel: a wrapped sum flips its sign
            i0, j0 = c["hot"][0][r], c["hot"][1][r]
            assert want[r, i0, j0] != 0 and np.sign(g[r, i0, j0]) == np.sign(want[r, i0, j0]), (placement, k, r)
    assert torch.equal(got[1], got[0] * 2.0 ** 20) and torch.equal(got[2], got[0] * 2.0 ** -20)
