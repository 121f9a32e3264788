"""Proposal index maps on the device (`ops.infer_index`, s2d_infer_index_u8): exact against the existing mask kernel under the rank
rule -- the two kernels evaluate one set of device functions, so the holding sets are the same bits -- and both rules against the
float64 restatement of tests/davis_index_refs.py outside its bands (module docstring there; the CPU module asserts the excluded
shares of these very inputs).  Then the named rows, the refusals, and inference_video(index_map=...)."""
import numpy as np
import pytest
import torch

from tests import davis_index_refs as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _dev(case_inputs):
    ml, dims, padded, img, out, query, score = case_inputs[:7]
    return (torch.from_numpy(ml).to(DEV), dims, padded, img, out, torch.from_numpy(query).to(DEV), torch.from_numpy(score).to(DEV))


def _first_hit(masks):
    """u8 planes [K, T, oh, ow] -> 1 + the first set k, 0 where none is set"""
    hold = masks != 0
    return torch.where(hold.any(0), hold.int().argmax(0) + 1, 0).to(torch.uint8)


@pytest.fixture(scope="module")
def inputs():
    cache = {}

    def get(case):
        if case["name"] not in cache:
            cache[case["name"]] = R.make_inputs(case)
        return cache[case["name"]]
    return get


@pytest.mark.parametrize("case", R.CASES, ids=R.CASE_IDS)
def test_rank_equals_first_hit_of_infer_masks(case, inputs):
    """byte for byte, a second call bitwise equal, the same bytes at an output pointer one byte off alignment, and the path
    (staged window or direct gather) the row is named for"""
    from s2d_amd import ops
    from s2d_amd._lib import lib
    ml, dims, padded, img, out, query, score = _dev(inputs(case))
    T, hm, wm = dims
    lds = lib().call("s2d_infer_index_lds_bytes", ml.shape[1], T, hm, wm, *padded, *img, *out, case["K"])
    assert (lds == 0) == case["name"].startswith("direct"), f"{case['name']}: {lds} bytes of LDS"
    masks, _ = ops.infer_masks(ml, dims, padded, img, out, query)
    want = _first_hit(masks)
    got = ops.infer_index(ml, dims, padded, img, out, query)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (T,) + tuple(out)
    assert torch.equal(got, want), f"{int((got != want).sum())} of {want.numel()} labels differ"
    assert torch.equal(ops.infer_index(ml, dims, padded, img, out, query, score, "rank"), got)
    n = got.numel()
    buf = torch.full((n + 8,), 0xEE, device=DEV, dtype=torch.uint8)
    lib().call("s2d_infer_index_u8", ml, ml.shape[1], T, hm, wm, *padded, *img, *out, query, None, case["K"], 0, buf[1:], ops._stream())
    assert torch.equal(buf[1:n + 1], got.flatten()) and int(buf[0]) == 0xEE and bool((buf[n + 1:] == 0xEE).all())


@pytest.mark.parametrize("rule", ["rank", "prob"])
@pytest.mark.parametrize("case", R.CASES, ids=R.CASE_IDS)
def test_both_rules_vs_float64(case, rule, inputs):
    from s2d_amd import ops
    host = inputs(case)
    ml, dims, padded, img, out, query, score = host
    planes = R.planes_of(ml, dims, query)
    v64 = R.two_stage(planes, padded, img, out)
    band = R.mask_band(planes, dims, padded, out)
    ref = R.index_from_values(v64, score, rule)
    excl = R.excluded(v64, band, score, rule)
    d = _dev(host)
    got = ops.infer_index(*d[:6], d[6], rule).cpu().numpy()
    share = excl.mean()
    wrong = int(((got != ref) & ~excl).sum())
    print(f"index row {case['name']} {rule}: band {band:.3e}, {int(excl.sum())} of {excl.size} pixels excluded (share {share:.3e}, cap "
          f"{R.CAP:.0e}), {wrong} wrong outside the band, {int((got != ref).sum())} differ in all")
    assert share <= R.CAP
    assert wrong == 0
    assert torch.equal(ops.infer_index(*d[:6], d[6], rule).cpu(), torch.from_numpy(got))            # second call


def test_rank_past_2_31_output_elements():
    """K = 2, 23 x 40 maps, T * 1080 * 1920 just over 2^31: the 64-bit output offsets, against infer_masks in frame chunks"""
    from s2d_amd import ops
    T, hm, wm, padded, img, out = 1036, 23, 40, (96, 160), (90, 160), (1080, 1920)
    assert T * out[0] * out[1] > 2 ** 31
    rng = np.random.default_rng(31)
    base = R.smooth_logits(rng, 2 * 8, hm, wm).reshape(2, 8, hm * wm)                    # 8 distinct frames, cycled
    ml = torch.zeros((T * hm * wm, 4), device=DEV)
    frames = torch.from_numpy(base).to(DEV)[:, torch.arange(T, device=DEV) % 8]          # [2, T, hm*wm]
    ml[:, 1], ml[:, 3] = frames[0].reshape(-1), frames[1].reshape(-1)
    query = torch.tensor([3, 1], device=DEV, dtype=torch.int32)
    got = ops.infer_index(ml, (T, hm, wm), padded, img, out, query)
    assert got.numel() > 2 ** 31
    step = 148
    for t0 in range(0, T, step):
        t1 = min(t0 + step, T)
        masks, _ = ops.infer_masks(ml[t0 * hm * wm:t1 * hm * wm], (t1 - t0, hm, wm), padded, img, out, query)
        assert torch.equal(got[t0:t1], _first_hit(masks)), f"frames {t0}..{t1}"
        del masks
    assert int(got[-1].max()) > 0                                                          # the frames past 2^31 were written


@pytest.mark.parametrize("rule", ["rank", "prob"])
@pytest.mark.parametrize("name", R.NAMED)
def test_named_rows(name, rule):
    from s2d_amd import ops
    row = R.named_inputs(name)
    d = _dev(row)
    got = ops.infer_index(*d[:6], d[6], rule).cpu().numpy()
    np.testing.assert_array_equal(got, row[7][rule])


def test_refusals_write_nothing():
    from s2d_amd import ops
    from s2d_amd._lib import lib
    ml, dims, padded, img, out, query, score = _dev(R.named_inputs("nested"))
    T, hm, wm = dims
    with pytest.raises(ValueError, match="score"):
        ops.infer_index(ml, dims, padded, img, out, query, None, "prob")
    with pytest.raises(ValueError):
        ops.infer_index(ml, dims, padded, img, out, query[:0].contiguous())
    with pytest.raises(ValueError):
        ops.infer_index(ml, dims, padded, img, out, torch.zeros(255, device=DEV, dtype=torch.int32))
    with pytest.raises(ValueError):
        ops.infer_index(ml[:, :6].contiguous(), dims, padded, img, out, query)
    with pytest.raises(ValueError):
        ops.infer_index(ml, dims, padded, img, out, query, score, "last")
    # the C ABI itself: S2D_ERR_ARG (a RuntimeError of the binding) and an untouched output
    n = T * out[0] * out[1]
    big = torch.zeros(255, device=DEV, dtype=torch.int32)
    bigs = torch.ones(255, device=DEV)
    for ldq, q, s, K, r in ((8, query, score, 0, 0), (8, big, bigs, 255, 0), (6, query, score, 2, 0), (8, query, None, 2, 1),
                            (8, query, score, 2, 2), (132, query, score, 2, 0)):
        buf = torch.full((n,), 0xEE, device=DEV, dtype=torch.uint8)
        with pytest.raises(RuntimeError, match="s2d_infer_index_u8"):
            lib().call("s2d_infer_index_u8", ml, ldq, T, hm, wm, *padded, *img, *out, q, s, K, r, buf, ops._stream())
        torch.cuda.synchronize()
        assert bool((buf == 0xEE).all())


def _video(seed, Q=12, C=1, T=3, hm=12, wm=16):
    rng = np.random.default_rng(seed)
    cls = torch.from_numpy(rng.normal(0, 2, (Q, C + 1)).astype(np.float32)).to(DEV)
    ml = np.zeros((T * hm * wm, 12), np.float32)
    ml[:, :Q] = R.smooth_logits(rng, Q * T, hm, wm).reshape(Q, T * hm * wm).T
    return cls, torch.from_numpy(ml).to(DEV), (T, hm, wm), (48, 64), (45, 61), (60, 80)


@pytest.mark.parametrize("rule", ["rank", "prob"])
@pytest.mark.parametrize("use_nms,threshold,max_proposals", [(False, 0.0, 20), (False, 0.4, 3), (True, 0.0, 4), (True, 0.3, 20)])
def test_inference_video_index_map(rule, use_nms, threshold, max_proposals):
    """labels <= max_proposals; the proposals are the host restatement's (threshold, NMS survivors, first max_proposals); the map
    is the index built from the planes the same call returns with device_masks=True"""
    from s2d_amd.modeling.postprocess import inference_video
    cls, ml, dims, padded, img, out = _video(5)
    N = 10
    planes = inference_video(cls, ml, dims, padded, img, out, N, use_nms, 0.5, device_masks=True)
    got = inference_video(cls, ml, dims, padded, img, out, N, use_nms, 0.5,
                          index_map={"rule": rule, "max_proposals": max_proposals, "score_threshold": threshold})
    assert got["pred_masks_format"] == "index_u8" and got["image_size"] == out
    index = got["pred_masks"]
    assert index.is_cuda and index.dtype == torch.uint8 and tuple(index.shape) == (dims[0],) + out
    assert int(index.max()) <= max_proposals
    # host restatement: the device_masks call kept (after its NMS over all N) scores in order; thresholding first and running the NMS
    # over the survivors keeps the same candidates among them, because a suppressed candidate suppresses nothing itself and the
    # thresholded ones are a suffix
    all_scores = planes["pred_scores"]
    keep = [i for i, s in enumerate(all_scores) if not s < threshold][:max_proposals]
    assert got["pred_scores"] == [all_scores[i] for i in keep] and got["pred_labels"] == [planes["pred_labels"][i] for i in keep]
    assert len(keep) >= 2
    sel = planes["pred_masks"][keep]
    if rule == "rank":
        want = _first_hit(sel)
        assert torch.equal(index, want)
    else:
        held = sel != 0
        assert bool(((index == 0) == ~held.any(0)).all())
        lab = index.long()
        inside = torch.gather(held, 0, (lab - 1).clamp(min=0)[None])[0] | (lab == 0)
        assert bool(inside.all())                                     # a label names a proposal that holds the pixel
        assert not torch.equal(index, _first_hit(sel))                # and the scores did decide some pixels


def test_index_map_refuses_rle_and_device_masks():
    from s2d_amd.modeling.postprocess import inference_video
    cls, ml, dims, padded, img, out = _video(6)
    for kw in ({"rle": True}, {"device_masks": True}):
        with pytest.raises(ValueError, match="index_map"):
            inference_video(cls, ml, dims, padded, img, out, 5, index_map={"rule": "rank"}, **kw)
    with pytest.raises(ValueError):
        inference_video(cls, ml, dims, padded, img, out, 5, index_map={"rule": "first"})
    with pytest.raises(ValueError):
        inference_video(cls, ml, dims, padded, img, out, 5, index_map={"max_proposals": 255})
