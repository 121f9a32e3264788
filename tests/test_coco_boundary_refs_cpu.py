"""CPU checks of COCO Boundary AP: the host-only plan call of the ragged band kernel (s2d_mask_boundary_ragged_plan: coverage,
prefix sums, LDS size, refusals), the worked case of boundary_refs.square_case on the references and through the product's host
matcher, and the driver's --iou-types flag.  No test here touches a device."""
import ctypes

import numpy as np
import pytest

from tests import boundary_refs as B
from tests import coco_boundary_refs as CB
from tests import coco_refs as R

PLAN_D = (1, 2, 16, 17, 32, 33, 60, 64)
ERR_ARG = -1                                                                   # S2D_ERR_ARG


@pytest.fixture(scope="module")
def dll():
    from s2d_amd.build import build
    lib = ctypes.CDLL(build(verbose=False))
    lib.s2d_mask_boundary_ragged_plan.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_long, ctypes.c_void_p, ctypes.c_void_p,
                                                  ctypes.c_void_p]
    lib.s2d_mask_boundary_ragged_plan.restype = ctypes.c_int
    return lib


def _plan(dll, spec, total, fill=-7):
    """-> (return code, plan [N, 12], n_workgroups, lds_bytes); the outputs prefilled with `fill`"""
    spec = np.ascontiguousarray(spec, np.int64).reshape(-1, 5)
    plan = np.full((len(spec), 12), fill, np.int64)
    nwg, lds = np.full(1, fill, np.int64), np.full(1, fill, np.int64)
    rc = dll.s2d_mask_boundary_ragged_plan(spec.ctypes.data, len(spec), total, plan.ctypes.data, nwg.ctypes.data, lds.ctypes.data)
    return rc, plan, int(nwg[0]), int(lds[0])


def _shapes():
    return dict(B.SHAPES, **CB.EXTRA_SHAPES)


def test_plan_covers_every_plane_row_and_word_exactly_once(dll):
    images = [(H, W, 1 + (n + k) % 3, d) for n, (H, W) in enumerate(_shapes().values()) for k, d in enumerate(PLAN_D)]
    assert len(images) == 13 * 8
    spec, total = CB.spec_of(images)
    rc, plan, nwg, lds = _plan(dll, spec, total)
    assert rc == 0
    assert np.array_equal(plan[:, :4], spec[:, :4])
    wg = 0
    lds_max = 0
    for row, (H, W, F, d) in zip(plan, images):
        word0, F_, H_, W_, dc, wpp, S, TW, TR, ntx, nty, wg0 = (int(v) for v in row)
        assert (F_, H_, W_) == (F, H, W) and dc == CB.clamp(H, W, d) and wpp == (H * W + 31) // 32 and S == (W + 31) // 32
        assert wg0 == wg                                                       # the exclusive prefix sum
        assert 1 <= TW <= 32 and TR >= 1
        count = np.zeros((F, H, S), np.int64)
        for b in range(F * ntx * nty):                                         # workgroup -> (plane, row tile, word tile), as the kernel
            f, t = divmod(b, ntx * nty)
            ty, tx = divmod(t, ntx)
            count[f, ty * TR:(ty + 1) * TR, tx * TW:(tx + 1) * TW] += 1
            assert ty * TR < H and tx * TW < S                                  # no tile lies wholly outside
        assert (count == 1).all(), (H, W, d)
        wg += F * ntx * nty
        need = 2 * TW * (TR + 2 * dc) * 4
        assert need <= 65536
        lds_max = max(lds_max, need)
        assert need == CB.plan_rule(H, W, d)[6]
    assert nwg == wg and lds == lds_max and lds <= 65536


def test_plan_named_shapes_keep_their_property(dll):
    H, W = CB.EXTRA_SHAPES["two_row_bands"]
    rc, plan, nwg, lds = _plan(dll, [[0, 1, H, W, 60]], (H * W + 31) // 32)
    assert rc == 0 and plan[0, 4] == 60 and plan[0, 10] >= 2 and plan[0, 8] * plan[0, 10] >= H
    H, W = CB.EXTRA_SHAPES["two_word_tiles"]
    rc, plan, nwg, lds = _plan(dll, [[0, 1, H, W, 7]], (H * W + 31) // 32)
    assert rc == 0 and plan[0, 9] == 2 and plan[0, 6] == 35 and plan[0, 7] * 2 >= 35
    assert CB.plan_rule(150, 1024, 60)[5] >= 2 and CB.plan_rule(21, 1100, 7)[4] == 2


@pytest.mark.parametrize("name,spec,total", [
    ("clamped_d_65", [[0, 1, 150, 140, 65]], 657),
    ("two_pow_31_pixels", [[0, 1, 1 << 16, 1 << 15, 2]], 1 << 26),
    ("negative_F", [[0, -1, 9, 33, 2]], 100),
    ("plane_past_total_words", [[0, 2, 9, 33, 2]], 19),
    ("overlapping_images", [[0, 2, 9, 33, 2], [10, 1, 9, 33, 2]], 100),
    ("descending_images", [[40, 1, 9, 33, 2], [0, 1, 9, 33, 2]], 100),
    ("zero_d", [[0, 1, 9, 33, 0]], 100),
    ("zero_height", [[0, 1, 0, 33, 1]], 100),
])
def test_plan_refusals_write_nothing(dll, name, spec, total):
    rc, plan, nwg, lds = _plan(dll, spec, total)
    assert rc == ERR_ARG, name
    assert (plan == -7).all() and nwg == -7 and lds == -7, name


def test_plan_refusal_cases_are_what_they_are_named_for():
    assert CB.clamp(150, 140, 65) == 65 and CB.clamp(150, 140, 72) == 70 and (150 * 140 + 31) // 32 == 657
    assert (1 << 16) * (1 << 15) == 1 << 31
    assert 2 * ((9 * 33 + 31) // 32) == 20                                       # two planes need 20 words: 19 are one short, and
    #                                                                              image 2 at word 10 starts inside image 1's 20


def test_plan_accepts_no_image_and_an_image_without_planes(dll):
    rc, plan, nwg, lds = _plan(dll, np.zeros((0, 5), np.int64), 0)
    assert rc == 0 and nwg == 0 and lds == 0
    wpp = (9 * 33 + 31) // 32
    spec = [[0, 2, 9, 33, 2], [2 * wpp, 0, 480, 640, 16], [2 * wpp, 3, 7, 5, 1]]
    rc, plan, nwg, lds = _plan(dll, spec, 2 * wpp + 3 * 2)
    assert rc == 0 and nwg == 5 and plan[:, 11].tolist() == [0, 2, 2]
    assert lds == 2 * 2 * (9 + 4) * 4                                           # the image without planes does not count: 9 x 33 at d = 2
    # the F = 0 image may also lie where an image left out has its words (the evaluator's chained fallback)
    spec = [[0, 2, 9, 33, 2], [2 * wpp, 0, 150, 140, 1], [2 * wpp + 2 * 657, 3, 7, 5, 1]]
    rc, plan, nwg, lds = _plan(dll, spec, 2 * wpp + 2 * 657 + 6)
    assert rc == 0 and nwg == 5


# ------------------------------------------------------------------------------------------------------------- worked case
WORKED = {0.02: (2, (152, 456), (152, 304), 0.0), 0.05: (5, (560, 840), (560, 700), 0.4)}


@pytest.mark.parametrize("ratio", [0.02, 0.05])
def test_worked_case_on_the_references(ratio):
    d, (bi, bu), (ci, cu), _ = WORKED[ratio]
    g, m = B.square_case()
    assert CB.dilation(64, 64, ratio) == d
    from s2d_amd.ytvis_eval import boundary_dilation
    assert boundary_dilation(64, 64, ratio) == d
    _, ad, ag, iou = R.mask_iou(m[None].astype(np.uint8), g[None].astype(np.uint8), [0])
    assert iou[0, 0] == 1520 / 1680 and ad[0] == ag[0] == 1600
    bd, bg = B.boundary_ref(m, d), B.boundary_ref(g, d)
    assert (int((bd & bg).sum()), int((bd | bg).sum())) == (bi, bu) and int(bd.sum()) == cu
    assert CB.band_iou_ref(m[None], g[None], [0], d)[0, 0] == bi / bu
    assert CB.band_iou_ref(m[None], g[None], [1], d)[0, 0] == ci / cu
    assert CB.min_iou_ref(m[None], g[None], [0], d)[0][0, 0] == min(1520 / 1680, bi / bu) == bi / bu


def _host_ap(iou, crowd=0):
    from s2d_amd.coco_eval import COCOEval
    doc, g, m = CB.square_doc(crowd)
    rec = {1: {"dt_ids": [1], "scores": [0.9], "labels": [1], "areas": [float(m.sum())], "ious": np.array([[iou]])}}
    ev = COCOEval(doc, iou_type="boundary").evaluate(rec, matcher="host").accumulate()
    assert ev.params.iouType == "boundary"
    return ev.summarize(out=None)


@pytest.mark.parametrize("ratio", [0.02, 0.05])
def test_worked_case_through_the_host_matcher(ratio):
    d, _, _, ap = WORKED[ratio]
    g, m = B.square_case()
    iou = CB.min_iou_ref(m[None], g[None], [0], d)[0][0, 0]
    stats = _host_ap(iou)
    # one true positive has precision tp / (tp + fp + eps) = 1 / (1 + 2^-52), so AP is k/10 of that: equal to k/10 within 1e-15
    assert abs(float(stats[0]) - ap) <= 1e-15 and (ap > 0 or stats[0] == 0.0)
    assert sum(iou >= t for t in R.IOU_THRS) == (0 if ratio == 0.02 else 4)     # 2/3: matched at 0.50 .. 0.65
    assert abs(float(_host_ap(1520 / 1680)[0]) - 0.9) <= 1e-15                  # the same pair without the min


# ----------------------------------------------------------------------------------------------------------------- driver
def test_driver_iou_types_flag():
    from s2d_amd.evaluate import parse_args, parse_iou_types, resolve_test_format
    base = ["--config-file", "c", "--gt", "g", "--image-root", "r", "--output-dir", "o"]
    a = parse_args(base)
    assert a.iou_types is None and parse_iou_types(a.iou_types) == ("segm", "bbox")
    a = parse_args(base + ["--iou-types", "segm,bbox,boundary", "--dilation-ratio", "0.05"])
    assert parse_iou_types(a.iou_types) == ("segm", "bbox", "boundary") and a.dilation_ratio == 0.05
    assert parse_iou_types("boundary") == ("boundary",)
    for bad in ("segm,mask", "", "segm,segm"):
        with pytest.raises(ValueError, match="iou-types"):
            parse_iou_types(bad)
    coco = {"images": [{"id": 1, "height": 4, "width": 4, "file_name": "a.jpg"}], "annotations": [], "categories": []}
    ytvis = {"videos": [], "annotations": []}
    assert resolve_test_format("auto", coco, iou_types=("segm", "boundary")) == "coco_image"
    assert resolve_test_format("auto", ytvis) == "ytvis"
    with pytest.raises(ValueError, match="iou-types"):
        resolve_test_format("auto", ytvis, iou_types=("segm", "bbox"))
    with pytest.raises(ValueError, match="boundary-ap"):
        resolve_test_format("auto", coco, boundary=True)
    with pytest.raises(ValueError, match="boundary-ap"):
        resolve_test_format("auto", coco, boundary=True, iou_types=("segm", "boundary"))


def test_evaluators_accept_boundary_and_refuse_unknown_types():
    from s2d_amd.coco_eval import COCOImageEvaluator, evaluate_coco
    doc, _, _ = CB.square_doc()
    ev = COCOImageEvaluator(json_file=doc, distributed=False, iou_types=("segm", "boundary"), dilation_ratio=0.05)
    assert ev._iou_types == ("segm", "boundary") and ev._dilation_ratio == 0.05
    assert COCOImageEvaluator(json_file=doc, distributed=False)._iou_types == ("segm", "bbox")
    with pytest.raises(ValueError, match="iou type"):
        COCOImageEvaluator(json_file=doc, iou_types=("segm", "contour"))
    with pytest.raises(ValueError, match="iou_type"):
        evaluate_coco(doc, [], iou_type="contour")
