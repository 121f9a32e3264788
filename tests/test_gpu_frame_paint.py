"""Stage-1 frame masks on the device (`ops.infer_frame_areas`, `ops.infer_paint`, `ops.paint_frames`; s2d_infer_frame_areas_i32,
s2d_infer_paint_u8).  Every assertion is an equality: the planes come from `ops.infer_masks` on the same inputs -- the kernels call
one set of device functions, so "proposal k holds the pixel" is the same bit -- and the picture painted from them is
tests/frame_masks_refs.paint_owner.  Then the named rows on constructed logits, the refusals, the memory bound and
inference_video(paint=...)."""
import numpy as np
import pytest
import torch

from tests import frame_masks_refs as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _dev(row):
    ml, dims, padded, img, out, query = row
    return torch.from_numpy(ml).to(DEV), dims, padded, img, out, torch.from_numpy(query).to(DEV)


@pytest.mark.parametrize("case", F.CASES, ids=F.CASE_IDS)
def test_areas_order_and_picture_equal_the_planes(case):
    from s2d_amd import ops
    from s2d_amd._lib import lib
    ml, dims, padded, img, out, query = d = _dev(F.make_inputs(case))
    T, hm, wm = dims
    K = case["K"]
    if case["name"].startswith("direct"):
        assert lib().call("s2d_infer_index_lds_bytes", ml.shape[1], T, hm, wm, *padded, *img, *out, K) == 0
    colors_h = F.case_colors(K)
    colors = torch.from_numpy(colors_h).to(DEV)
    masks, _ = ops.infer_masks(*d)
    masks_h = masks.cpu().numpy()

    areas, order = ops.infer_frame_areas(*d)
    assert areas.dtype == torch.int32 and tuple(areas.shape) == (K, T) and tuple(order.shape) == (T, K)
    want_areas = masks_h.astype(np.int64).sum((2, 3))
    np.testing.assert_array_equal(areas.cpu().numpy(), want_areas)
    np.testing.assert_array_equal(order.cpu().numpy(), np.argsort(-want_areas.T, axis=1, kind="stable"))
    assert ops.infer_frame_areas(*d, want_order=False)[1] is None

    rgb, index = ops.infer_paint(*d, order, colors)
    assert rgb.dtype == torch.uint8 and tuple(rgb.shape) == (T,) + tuple(out) + (3,) and tuple(index.shape) == (T,) + tuple(out)
    want_rgb, want_index = F.paint_owner(masks_h, colors_h)
    np.testing.assert_array_equal(index.cpu().numpy(), want_index)
    np.testing.assert_array_equal(rgb.cpu().numpy(), want_rgb)
    overlay, _ = ops.render_instances(torch.zeros_like(rgb), masks, order, colors, alpha=256)
    assert torch.equal(rgb, overlay)
    assert ops.infer_paint(*d, order, colors, want_index=False)[1] is None

    # a second call of both: bitwise equal
    rgb2, index2, areas2, order2 = ops.paint_frames(*d, colors)
    assert torch.equal(areas2, areas) and torch.equal(order2, order) and torch.equal(rgb2, rgb) and torch.equal(index2, index)

    # rgb (and index) one byte off alignment: the byte-store path, and nothing written outside
    n = index.numel()
    buf = torch.full((3 * n + 8,), 0xEE, device=DEV, dtype=torch.uint8)
    ibuf = torch.full((n + 8,), 0xEE, device=DEV, dtype=torch.uint8)
    lib().call("s2d_infer_paint_u8", ml, ml.shape[1], T, hm, wm, *padded, *img, *out, query, K, order, colors, buf[1:], ibuf[1:],
               ops._stream())
    assert torch.equal(buf[1:3 * n + 1], rgb.flatten()) and int(buf[0]) == 0xEE and bool((buf[3 * n + 1:] == 0xEE).all())
    assert torch.equal(ibuf[1:n + 1], index.flatten()) and int(ibuf[0]) == 0xEE and bool((ibuf[n + 1:] == 0xEE).all())


@pytest.mark.parametrize("name", F.NAMED)
def test_named_rows(name):
    from s2d_amd import ops
    d = _dev(F.named_inputs(name))
    K = d[5].shape[0]
    colors_h = F.case_colors(K)
    masks_h = ops.infer_masks(*d)[0].cpu().numpy()
    rgb, index, areas, order = ops.paint_frames(*d, torch.from_numpy(colors_h).to(DEV))
    np.testing.assert_array_equal(areas.cpu().numpy(), F.plane_areas(masks_h))
    np.testing.assert_array_equal(order.cpu().numpy(), F.stable_order(F.plane_areas(masks_h)))
    want_rgb, want_index = F.paint_owner(masks_h, colors_h)
    np.testing.assert_array_equal(rgb.cpu().numpy(), want_rgb)
    np.testing.assert_array_equal(index.cpu().numpy(), want_index)
    F.check_named_property(name, masks_h != 0, rgb.cpu().numpy(), index.cpu().numpy(), colors_h)


def test_order_entries_out_of_range_are_clamped():
    """a row that is no permutation: unspecified colours, but every label names a proposal and nothing outside the outputs is
    written"""
    from s2d_amd import ops
    d = _dev(F.named_inputs("nested"))
    T, K = d[1][0], d[5].shape[0]
    colors = torch.from_numpy(F.case_colors(K)).to(DEV)
    order = torch.tensor([[-7, 2 ** 30]] * T, device=DEV, dtype=torch.int32)
    rgb, index = ops.infer_paint(*d, order, colors)
    assert int(index.max()) <= K
    held = ops.infer_masks(*d)[0].any(0)
    assert torch.equal(index != 0, held)


def test_refusals():
    from s2d_amd import ops
    from s2d_amd._lib import lib
    ml, dims, padded, img, out, query = d = _dev(F.named_inputs("nested"))
    T, hm, wm = dims
    K = query.shape[0]
    colors = torch.from_numpy(F.case_colors(K)).to(DEV)
    _, order = ops.infer_frame_areas(*d)
    big = torch.zeros(255, device=DEV, dtype=torch.int32)
    for q in (query[:0].contiguous(), big):
        with pytest.raises(ValueError, match="proposals"):
            ops.infer_frame_areas(ml, dims, padded, img, out, q)
        with pytest.raises(ValueError, match="proposals"):
            ops.infer_paint(ml, dims, padded, img, out, q, order, colors)
    with pytest.raises(ValueError, match="ldq"):
        ops.infer_frame_areas(ml[:, :6].contiguous(), dims, padded, img, out, query)
    with pytest.raises(ValueError, match="ldq"):
        ops.infer_paint(ml[:, :6].contiguous(), dims, padded, img, out, query, order, colors)
    with pytest.raises(ValueError, match="order"):
        ops.infer_paint(*d, order.t().contiguous(), colors)
    with pytest.raises(ValueError, match="order"):
        ops.infer_paint(*d, order[:, :1].contiguous(), colors)
    with pytest.raises(ValueError, match="colors"):
        ops.infer_paint(*d, order, colors.int())
    with pytest.raises(ValueError, match="colors"):
        ops.infer_paint(*d, order, colors[:1].contiguous())
    # the C ABI itself: S2D_ERR_ARG (a RuntimeError of the binding) and untouched outputs
    n = T * out[0] * out[1]
    order255, colors255 = torch.zeros((T, 255), device=DEV, dtype=torch.int32), torch.ones((255, 3), device=DEV, dtype=torch.uint8)
    for ldq, q, k in ((8, query, 0), (8, big, 255), (6, query, K), (132, query, K)):
        a = torch.full((255 * T,), -5, device=DEV, dtype=torch.int32)
        o = torch.full((255 * T,), -5, device=DEV, dtype=torch.int32)
        with pytest.raises(RuntimeError, match="s2d_infer_frame_areas_i32"):
            lib().call("s2d_infer_frame_areas_i32", ml, ldq, T, hm, wm, *padded, *img, *out, q, k, a, o, ops._stream())
        buf = torch.full((3 * n,), 0xEE, device=DEV, dtype=torch.uint8)
        ibuf = torch.full((n,), 0xEE, device=DEV, dtype=torch.uint8)
        with pytest.raises(RuntimeError, match="s2d_infer_paint_u8"):
            lib().call("s2d_infer_paint_u8", ml, ldq, T, hm, wm, *padded, *img, *out, q, k, order255, colors255, buf, ibuf,
                       ops._stream())
        torch.cuda.synchronize()
        assert bool((a == -5).all()) and bool((o == -5).all()) and bool((buf == 0xEE).all()) and bool((ibuf == 0xEE).all())


def test_no_plane_sized_tensor_is_allocated():
    """K = 50, T = 2, out 120 x 160: peak memory grows by at most the outputs (rgb + index + areas + order) + 64 KiB; the planes alone
    would be 1.9 MB"""
    from s2d_amd import ops
    K, T, hm, wm, padded, img, out = 50, 2, 23, 30, (92, 120), (90, 120), (120, 160)
    rng = np.random.default_rng(3)
    ml = np.zeros((T * hm * wm, 128), np.float32)
    ml[:, :100] = F.R.smooth_logits(rng, 100 * T, hm, wm).reshape(100, T * hm * wm).T
    ml = torch.from_numpy(ml).to(DEV)
    query = torch.arange(K, device=DEV, dtype=torch.int32)
    colors = torch.from_numpy(F.case_colors(K)).to(DEV)
    ops.paint_frames(ml, (T, hm, wm), padded, img, out, query, colors)            # library and kernels loaded before measuring
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    rgb, index, areas, order = ops.paint_frames(ml, (T, hm, wm), padded, img, out, query, colors)
    torch.cuda.synchronize()
    grown = torch.cuda.max_memory_allocated() - before
    outputs = sum(t.numel() * t.element_size() for t in (rgb, index, areas, order))
    print(f"paint_frames K = {K}, T = {T}, out {out}: peak grew by {grown} bytes, outputs {outputs} bytes, planes {K * T * out[0] * out[1]}")
    assert K * T * out[0] * out[1] > outputs + 65536
    assert grown <= outputs + 65536
    assert int(areas.max()) > 0 and int(index.max()) > 1


def _video(seed, Q=12, C=1, T=3, hm=12, wm=16):
    rng = np.random.default_rng(seed)
    cls = torch.from_numpy(rng.normal(0, 2, (Q, C + 1)).astype(np.float32)).to(DEV)
    ml = np.zeros((T * hm * wm, 12), np.float32)
    ml[:, :Q] = F.R.smooth_logits(rng, Q * T, hm, wm).reshape(Q, T * hm * wm).T
    return cls, torch.from_numpy(ml).to(DEV), (T, hm, wm), (48, 64), (45, 61), (60, 80)


@pytest.mark.parametrize("use_nms,threshold,max_masks", [(False, 0.0, 50), (False, 0.4, 3), (True, 0.0, 4), (True, 0.3, 50)])
def test_inference_video_paint(use_nms, threshold, max_masks):
    """the proposals are those of index_map with the same threshold and count (one selection); the picture is paint_owner of the
    planes the device_masks call returns for them, in the default colours"""
    from s2d_amd import ops
    from s2d_amd.modeling.postprocess import inference_video
    cls, ml, dims, padded, img, out = _video(5)
    N = 10
    planes = inference_video(cls, ml, dims, padded, img, out, N, use_nms, 0.5, device_masks=True)
    ref = inference_video(cls, ml, dims, padded, img, out, N, use_nms, 0.5,
                          index_map={"rule": "rank", "max_proposals": max_masks, "score_threshold": threshold})
    got = inference_video(cls, ml, dims, padded, img, out, N, use_nms, 0.5, paint={"max_masks": max_masks, "score_threshold": threshold})
    assert got["pred_masks_format"] == "rgb_u8" and got["image_size"] == out
    assert got["pred_scores"] == ref["pred_scores"] and got["pred_labels"] == ref["pred_labels"]
    keep = [i for i, s in enumerate(planes["pred_scores"]) if not s < threshold][:max_masks]
    assert got["pred_scores"] == [planes["pred_scores"][i] for i in keep] and len(keep) >= 2
    sel = planes["pred_masks"][keep].cpu().numpy()
    want_rgb, want_index = F.paint_owner(sel, ops.mask_colors(max_masks))
    rgb, index = got["pred_masks"], got["pred_index"]
    assert rgb.is_cuda and rgb.dtype == torch.uint8 and tuple(rgb.shape) == (dims[0],) + out + (3,)
    np.testing.assert_array_equal(rgb.cpu().numpy(), want_rgb)
    np.testing.assert_array_equal(index.cpu().numpy(), want_index)
    assert got["pred_areas"] == F.plane_areas(sel).tolist()


def test_inference_video_paint_without_proposals_is_black():
    from s2d_amd.modeling.postprocess import inference_video
    cls, ml, dims, padded, img, out = _video(6)
    got = inference_video(cls, ml, dims, padded, img, out, 5, paint={"score_threshold": 2.0})
    assert got["pred_scores"] == [] and got["pred_areas"] == [] and got["pred_masks_format"] == "rgb_u8"
    assert tuple(got["pred_masks"].shape) == (dims[0],) + out + (3,) and not bool(got["pred_masks"].any())
    assert tuple(got["pred_index"].shape) == (dims[0],) + out and not bool(got["pred_index"].any())
