"""Eval-side step after the path: `inference_video` of both meta-architectures
(model_training/mask2former_video/kd_video_maskformer_model.py:530-610, video_maskformer_model.py:298-360) on the
device kernels of csrc/infer.hip.  The python side keeps only what the reference keeps on the host: the greedy loop over
K <= a few hundred candidates (on the K x K integer counts, not on the masks) and the final lists."""
import numpy as np
import torch

from .. import ops
from ..index_components import COMPONENT_KEYS, FILL_KEYS


def greedy_mask_nms(inter, labels, thr):
    """:552-583 on the pairwise counts: inter [K,K] int64 numpy (diagonal = areas), labels [K]; candidates are already in
    descending score order.  IoU = float32(sum(a & b)) / float32(sum(a | b)) as the reference forms it, 0 if the union is
    empty; a later same-label candidate is suppressed when IoU > thr."""
    K = inter.shape[0]
    area = np.diagonal(inter)
    alive = list(range(K))
    keep = []
    thr = np.float32(thr)
    while alive:
        cur = alive.pop(0)
        keep.append(cur)
        rem = []
        for o in alive:
            if labels[o] != labels[cur]:
                rem.append(o)
                continue
            i = np.float32(inter[cur, o])
            u = np.float32(area[cur] + area[o] - inter[cur, o])
            iou = i / u if u > 0 else np.float32(0.0)
            if iou <= thr:
                rem.append(o)
        alive = rem
    return keep


def index_map_options(index_map):
    """{"rule", "max_proposals", "score_threshold"} with the defaults ("rank", 20, 0.0) filled in; unknown keys, rules and proposal
    counts outside 1..254 are refused.  The component cleanup keys (ops.component_options: min_component_area, keep_largest,
    component_connectivity) and the hole-filling key (ops.fill_options: fill_holes) are known too and checked here; they are no part
    of the returned tuple."""
    opts = {"rule": "rank", "max_proposals": 20, "score_threshold": 0.0}
    unknown = set(index_map) - set(opts) - set(COMPONENT_KEYS) - set(FILL_KEYS)
    if unknown:
        raise ValueError(f"index_map keys {sorted(unknown)}: rule, max_proposals, score_threshold and {', '.join(COMPONENT_KEYS)} "
                         f"are known, and {', '.join(FILL_KEYS)}")
    ops.component_options(index_map)
    ops.fill_options(index_map)
    opts.update(index_map)
    if opts["rule"] not in ops.INDEX_RULES:
        raise ValueError(f"index_map rule {opts['rule']!r}: one of {', '.join(ops.INDEX_RULES)}")
    if not 1 <= int(opts["max_proposals"]) <= ops.INDEX_MAX_PROPOSALS:
        raise ValueError(f"index_map max_proposals = {opts['max_proposals']}: 1..{ops.INDEX_MAX_PROPOSALS} (label 255 is void)")
    return opts["rule"], int(opts["max_proposals"]), float(opts["score_threshold"])


def _select_proposals(class_logits, mask_logits, dims, padded, img_size, out_size, num_predictions, use_nms, nms_threshold, threshold,
                      max_proposals):
    """the proposals of the plane-free outputs (index_map, paint): infer_select's top num_predictions, without those scored below the
    threshold, (use_nms) without those the greedy mask-NMS suppresses -- the only step that still needs bit planes, of the
    thresholded candidates -- and of the rest the first max_proposals -> (scores, query, label) on the device, or None for none"""
    sel = []
    if class_logits.shape[0]:
        scores, query, label = ops.infer_select(class_logits, num_predictions)
        n = int((~(scores < threshold)).sum())                       # the scores descend: a prefix
        sel = list(range(n))
        if use_nms and n:
            _, bits = ops.infer_masks(mask_logits, dims, padded, img_size, out_size, query[:n].contiguous(), want_bits=True)
            sel = greedy_mask_nms(ops.mask_pair_counts(bits).cpu().numpy(), label[:n].cpu().numpy(), nms_threshold)
        sel = sel[:max_proposals]
    if not sel:
        return None
    idx = torch.as_tensor(sel, device=mask_logits.device, dtype=torch.long)
    return scores[idx].contiguous(), query[idx].contiguous(), label[idx]


def _inference_index(class_logits, mask_logits, dims, padded, img_size, out_size, num_predictions, use_nms, nms_threshold, index_map):
    """inference_video(index_map=...): the proposals of _select_proposals; label p + 1 of the map is pred_scores[p]"""
    rule, max_proposals, threshold = index_map_options(index_map)
    picked = _select_proposals(class_logits, mask_logits, dims, padded, img_size, out_size, num_predictions, use_nms, nms_threshold,
                               threshold, max_proposals)
    if picked is None:
        index = torch.zeros((dims[0],) + tuple(out_size), device=mask_logits.device, dtype=torch.uint8)
        return {"image_size": tuple(out_size), "pred_scores": [], "pred_labels": [], "pred_masks": index, "pred_masks_format": "index_u8"}
    scores, query, label = picked
    index = ops.infer_index(mask_logits, dims, padded, img_size, out_size, query, scores, rule)
    out = {"image_size": tuple(out_size), "pred_scores": scores.tolist(), "pred_labels": label.tolist(), "pred_masks": index,
           "pred_masks_format": "index_u8"}
    min_area, largest, conn = ops.component_options(index_map)
    if min_area > 0 or largest:                                      # off: nothing is launched and no key is added
        _, removed = ops.filter_components(index, min_area, largest, conn, out=index)
        out["pred_removed"] = removed
    max_hole = ops.fill_options(index_map)
    if max_hole > 0:                                                 # fill(filter(map)); off: nothing is launched, no key is added
        _, filled = ops.fill_index_holes(index, max_hole, conn, out=index)
        out["pred_filled"] = filled
    return out


def paint_options(paint):
    """{"max_masks", "score_threshold", "colors"} with the defaults (50, 0.35, None: ops.mask_colors) filled in; unknown keys, mask
    counts outside 1..254 and a colour table that is not u8 [>= max_masks, 3] are refused.  The component cleanup keys
    (ops.component_options: min_component_area, keep_largest, component_connectivity) and the hole-filling key (ops.fill_options:
    fill_holes) are known too and checked here; they are no part of the returned tuple."""
    opts = {"max_masks": 50, "score_threshold": 0.35, "colors": None}
    unknown = set(paint) - set(opts) - set(COMPONENT_KEYS) - set(FILL_KEYS)
    if unknown:
        raise ValueError(f"paint keys {sorted(unknown)}: max_masks, score_threshold, colors and {', '.join(COMPONENT_KEYS)} are known, "
                         f"and {', '.join(FILL_KEYS)}")
    ops.component_options(paint)
    ops.fill_options(paint)
    opts.update(paint)
    max_masks = int(opts["max_masks"])
    if not 1 <= max_masks <= ops.PAINT_MAX_PROPOSALS:
        raise ValueError(f"paint max_masks = {opts['max_masks']}: 1..{ops.PAINT_MAX_PROPOSALS}")
    colors = ops.mask_colors(max_masks) if opts["colors"] is None else np.asarray(opts["colors"])
    if colors.dtype != np.uint8 or colors.ndim != 2 or colors.shape[1] != 3 or colors.shape[0] < max_masks:
        raise ValueError(f"paint colors must be uint8 [>= {max_masks}, 3], got {colors.dtype} {colors.shape}")
    return max_masks, float(opts["score_threshold"]), colors


def _inference_paint(class_logits, mask_logits, dims, padded, img_size, out_size, num_predictions, use_nms, nms_threshold, paint):
    """inference_video(paint=...): the proposals of _select_proposals painted by ops.paint_frames; colour p of the table and label
    p + 1 of pred_index are pred_scores[p]"""
    max_masks, threshold, colors = paint_options(paint)
    dev = mask_logits.device
    picked = _select_proposals(class_logits, mask_logits, dims, padded, img_size, out_size, num_predictions, use_nms, nms_threshold,
                               threshold, max_masks)
    if picked is None:
        shape = (dims[0],) + tuple(out_size)
        return {"image_size": tuple(out_size), "pred_scores": [], "pred_labels": [], "pred_areas": [],
                "pred_masks": torch.zeros(shape + (3,), device=dev, dtype=torch.uint8),
                "pred_index": torch.zeros(shape, device=dev, dtype=torch.uint8), "pred_masks_format": "rgb_u8"}
    scores, query, label = picked
    table = torch.from_numpy(np.ascontiguousarray(colors[:query.shape[0]])).to(dev)
    rgb, index, areas, _ = ops.paint_frames(mask_logits, dims, padded, img_size, out_size, query, table)
    out = {"image_size": tuple(out_size), "pred_scores": scores.tolist(), "pred_labels": label.tolist(), "pred_areas": areas.tolist(),
           "pred_masks": rgb, "pred_index": index, "pred_masks_format": "rgb_u8"}
    min_area, largest, conn = ops.component_options(paint)
    if min_area > 0 or largest:                                      # off: nothing is launched and no key is added
        # a removed pixel becomes black even where a larger instance painted underneath also holds it: the paint keeps no second
        # owner.  pred_areas stay the areas the draw order was decided by
        _, removed = ops.filter_components(index, min_area, largest, conn, rgb=rgb, out=index)
        out["pred_removed"] = removed
    max_hole = ops.fill_options(paint)
    if max_hole > 0:                                                 # fill(filter(map)): a filled pixel takes its owner's colour
        _, filled = ops.fill_index_holes(index, max_hole, conn, rgb=rgb, colors=table, out=index)
        out["pred_filled"] = filled
    return out


@torch.no_grad()
def inference_video(class_logits, mask_logits, dims, padded, img_size, out_size, num_predictions, use_nms=False,
                    nms_threshold=0.75, rle=False, device_masks=False, index_map=None, paint=None):
    """class_logits [Q,C+1]; mask_logits pixel-major [T*hm*wm, ldq] of ONE video; dims = (T, hm, wm); padded = network
    input size (Hp,Wp), img_size = size without padding, out_size = (height, width) of the original video.
    Returns the reference's dict: image_size, pred_scores (list of float), pred_labels (list of int), pred_masks (list of
    CPU bool tensors [T,H,W]).  rle=True: the masks stay on the device and `pred_masks` holds, per prediction, the list of T
    COCO RLE dicts that instances_to_coco_json_video (data_video/ytvis_eval.py:345-350) would build from them.
    device_masks=True: `pred_masks` is the CUDA u8 tensor [K,T,H,W] (0 / 1, after NMS) with "pred_masks_format": "device_u8".
    index_map={"rule": "rank" | "prob", "max_proposals": 20, "score_threshold": 0.0}: `pred_masks` is ONE CUDA u8 tensor [T,H,W]
    of non-overlapping proposal labels (0: none, p + 1: the proposal of pred_scores[p]; ops.infer_index), "pred_masks_format":
    "index_u8"; not together with rle / device_masks.
    paint={"max_masks": 50, "score_threshold": 0.35, "colors": None}: the stage-1 pseudo-mask picture (ops.paint_frames): `pred_masks`
    is the CUDA u8 RGB tensor [T,H,W,3] ("pred_masks_format": "rgb_u8"), `pred_index` the u8 [T,H,W] owner map (p + 1: the proposal of
    pred_scores[p]), `pred_areas` K lists of T pixel counts; not together with rle / device_masks / index_map.
    Both dicts also take "min_component_area": 0, "keep_largest": False, "component_connectivity": 8 (ops.filter_components): with an
    area above 0 or keep_largest the map is cleaned in place -- in the picture the removed pixels become black -- and `pred_removed`
    is the CUDA int32 [T] count of removed pixels per frame; with the defaults nothing is launched and the key is absent.
    Both also take "fill_holes": 0 | N | "all" (ops.fill_index_holes, applied after the cleanup): every zero region of at most N
    pixels that does not touch the frame border and is enclosed by ONE instance takes that instance's id -- and its colour in the
    picture -- and `pred_filled` is the CUDA int32 [T] count of filled pixels per frame; with 0 nothing is launched and the key is
    absent."""
    if paint is not None:
        if rle or device_masks or index_map is not None:
            raise ValueError("paint replaces pred_masks by one RGB picture per frame: it does not combine with rle / device_masks / "
                             "index_map")
        return _inference_paint(class_logits, mask_logits, dims, padded, img_size, out_size, num_predictions, use_nms, nms_threshold,
                                paint)
    if index_map is not None:
        if rle or device_masks:
            raise ValueError("index_map replaces pred_masks by one label map: it does not combine with rle / device_masks")
        return _inference_index(class_logits, mask_logits, dims, padded, img_size, out_size, num_predictions, use_nms, nms_threshold,
                                index_map)
    if class_logits.shape[0] == 0:                                   # :584-587
        return {"image_size": tuple(out_size), "pred_scores": [], "pred_labels": [], "pred_masks": []}
    scores, query, label = ops.infer_select(class_logits, num_predictions)
    masks, bits = ops.infer_masks(mask_logits, dims, padded, img_size, out_size, query, want_bits=use_nms)
    if use_nms:
        inter = ops.mask_pair_counts(bits).cpu().numpy()
        labels_h = label.cpu().numpy()
        keep = greedy_mask_nms(inter, labels_h, nms_threshold)
        sel = torch.as_tensor(keep, device=masks.device, dtype=torch.long)
        masks, scores, label = masks[sel], scores[sel], label[sel]
    if device_masks:
        return {"image_size": tuple(out_size), "pred_scores": scores.tolist(), "pred_labels": label.tolist(),
                "pred_masks": masks, "pred_masks_format": "device_u8"}
    if rle:
        from ..rle import encode_video_predictions
        return {"image_size": tuple(out_size), "pred_scores": scores.tolist(), "pred_labels": label.tolist(),
                "pred_masks": encode_video_predictions(masks), "pred_masks_format": "coco_rle"}
    masks_h = torch.empty(masks.shape, dtype=torch.uint8, pin_memory=True)   # pinned: the copy runs at PCIe rate, not pageable rate
    masks_h.copy_(masks, non_blocking=True)
    torch.cuda.current_stream().synchronize()
    masks_h = masks_h.view(torch.bool)
    return {"image_size": tuple(out_size), "pred_scores": scores.tolist(), "pred_labels": label.tolist(),
            "pred_masks": [m for m in masks_h]}
