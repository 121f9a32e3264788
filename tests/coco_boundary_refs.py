"""References for the COCO Boundary AP tests.  None restates the kernel: the bands come from scipy's morphology on bool images
(boundary_refs.boundary_ref), the counts are Python integers, the dataset reference is coco_refs.evaluate_dataset on the minimum of
the two IoU matrices.  plan_rule restates the tile rule of s2d_mask_boundary_ragged_plan and is used to check that the library's
plan covers every plane exactly once, not to compare the table column by column."""
import numpy as np

from tests import coco_refs as R
from tests.boundary_refs import boundary_ref

EXTRA_SHAPES = {"two_word_tiles": (21, 1100), "two_row_bands": (150, 1024), "vga": (480, 640)}


def dilation(H, W, ratio):
    """max(1, round(ratio * diagonal)), Python's round"""
    return max(1, int(round(ratio * (H * H + W * W) ** 0.5)))


def clamp(H, W, d):
    return min(d, (min(H, W) + 1) // 2)


def band_iou_ref(dt, gt, crowd, d):
    """bool / uint8 masks dt [D, H, W], gt [G, H, W], G crowd flags, erosion count d -> float64 [D, G]: the IoU of the boundary
    bands, |Bd & Bg| / |Bd | Bg|, or / |Bd| against a crowd, 0 where the denominator is 0"""
    bd = [boundary_ref(np.asarray(m, bool), d) for m in dt]
    bg = [boundary_ref(np.asarray(m, bool), d) for m in gt]
    out = np.zeros((len(bd), len(bg)), np.float64)
    for i, a in enumerate(bd):
        for j, b in enumerate(bg):
            n = int(np.count_nonzero(a & b))
            u = int(np.count_nonzero(a)) if crowd[j] else int(np.count_nonzero(a | b))
            out[i, j] = np.float64(n) / np.float64(u) if u > 0 else 0.0
    return out


def min_iou_ref(dt, gt, crowd, d):
    """-> (min(mask IoU, band IoU) [D, G], mask areas of dt, of gt)"""
    D, G = len(dt), len(gt)
    if D == 0 or G == 0:
        _, ad, ag, _ = R.mask_iou(np.asarray(dt, np.uint8), np.asarray(gt, np.uint8), crowd)
        return np.zeros((D, G)), ad, ag
    _, ad, ag, iou = R.mask_iou(np.asarray(dt, np.uint8), np.asarray(gt, np.uint8), crowd)
    return np.minimum(iou, band_iou_ref(dt, gt, crowd, d)), ad, ag


def plan_rule(H, W, d):
    """-> (clamped d, S, TW, TR, ntx, nty, lds bytes) of one image, from the rule the header documents"""
    d = clamp(H, W, d)
    S = (W + 31) // 32
    ntx = (S + 31) // 32
    TW = (S + ntx - 1) // ntx
    tr_max = 8192 // TW - 2 * d
    nty = (H + tr_max - 1) // tr_max
    TR = (H + nty - 1) // nty
    return d, S, TW, TR, ntx, nty, 2 * TW * (TR + 2 * d) * 4


def spec_of(shapes_F_d):
    """[(H, W, F, d)] -> (spec int64 [N, 5] with the planes back to back, total words)"""
    spec, word = [], 0
    for H, W, F, d in shapes_F_d:
        spec.append([word, F, H, W, d])
        word += F * ((H * W + 31) // 32)
    return np.asarray(spec, np.int64).reshape(-1, 5), word


def square_doc(crowd=0):
    """the worked case as a COCO document with one ground truth (area from the mask) -> (doc, gt image, detection image)"""
    from tests.boundary_refs import square_case
    g, d = square_case()
    doc = {"images": [{"id": 1, "height": 64, "width": 64, "file_name": "1.jpg"}], "categories": [{"id": 1, "name": "fg"}],
           "annotations": [{"id": 1, "image_id": 1, "category_id": 1, "iscrowd": crowd, "area": float(g.sum())}]}
    return doc, g, d
