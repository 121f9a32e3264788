"""Image self-training rounds: the previous round's annotation file + this round's predictions -> the next round's annotation file.

    python -m s2d_amd.selftrain --new-pred OUT/coco_instances_results.json --prev-ann round0.json --save-path round1.json [--threshold 0.7]
        [--min-component-area N] [--keep-largest] [--fill-holes N|all] [--component-connectivity 4|8]

The step that closes the image loop (train --train-format coco_image -> evaluate --test-format coco_image -> selftrain -> train), as
keymask.results_to_annotations closes the video loop.  Restates the reference's model_training/cutler/tools/get_self_training_ann.py
with its flags, defaults and observable behaviour:

  * predictions with score >= threshold are grouped by image_id in file order; previous annotations are grouped by image_id in file
    order;
  * for each image with previous annotations, in order of its first appearance among them: without a kept prediction all its previous
    annotations are kept; otherwise its predictions come first, then the previous annotations whose IoU with EVERY kept prediction of
    the image is below 0.5, both in their own order;
  * then the predictions of images without a previous annotation, in order of first appearance;
  * every output annotation gets id = 1.., iscrowd = 0, area = bbox[2] * bbox[3] (the box area, not the mask's), and
    width = segmentation.size[0], height = segmentation.size[1].  COCO RLE sizes are [height, width], so THE TWO ARE SWAPPED; that is
    the reference's output and it is kept (nothing in the project reads them).  Prediction entries keep their other fields, `score`
    included;
  * `images` is the previous file's list.

Device side, per chunk of images of different sizes (bounded by CHUNK_WORDS / CHUNK_IMAGES, coco_eval's limits) five library calls
however many images the chunk holds: the ragged RLE parse, decode and tight boxes (rle_ragged.decode_ragged), the mask IoU
(s2d_coco_mask_iou_ragged: previous masks as the D side, kept predictions as the G side, no crowd) and the keep rule
(s2d_selftrain_keep_ragged), then ONE read-back of the keep flags and the boxes.  Only images that need it enter a chunk: those with
both kinds of mask, and those with an entry that lacks a `bbox`.  A polygon segmentation costs one more call per image that has any.
RLE and polygon decode are restated from pycocotools (absent from the project's machines): parity unpinned; polygons are filled by the
library's centre-sample even-odd rule (data/image_clip.py).

Where this differs from the reference, on purpose:
  * a missing `bbox` (the project's own coco_instances_results.json entries have none; the reference raises KeyError on them) is filled
    with the mask's tight box, a float [x, y, w, h]; an existing `bbox` is left alone;
  * `categories`, `info` and `licenses` are the previous file's when it has them; without `categories` the reference's single
    {"id": 1, "name": "fg", "supercategory": "fg"} is written; `info` / `licenses` the previous file lacks are left out (the
    reference writes its own ImageNet-1K texts whatever the data is);
  * a merged annotation whose category_id is not among the output categories is refused, naming the image: the next round's
    load_coco_image_train would fail on it far from the cause;
  * the reference swallows any exception per image and silently keeps the old masks.  Here an RLE whose size is not its image's, an
    entry for an image absent from `images`, or an entry without a segmentation is a ValueError that names the image;
  * the keep rule is decided in integers: 2 * inter < union with union = area_d + area_g - inter.  For images of fewer than 2^24
    pixels that is exactly the reference's float32 `inter / union < 0.5` (both counts are exact in float32; a quotient below one half is at most
    1/2 - 1/(2 union) < 1/2 - 2^-25, the float32 next below 0.5, so rounding cannot lift it to 0.5, and one at or above one half
    cannot round below it); a pair of two empty masks has union 0, the reference's
    NaN compares false, and the previous mask is dropped here too;
  * a polygon segmentation has no `size`: width / height take the image's [height, width] in the same swapped order (the reference
    cannot merge polygons at all: it indexes segmentation["size"]);
  * the inputs are not modified: output annotations are copies;
  * the mask cleanup options (s2d_amd/clean_annotations.py; this project's own, off by default) clean the merged document's masks
    just before it is written.  The merge and keep rules see the masks as they came, and with the options off the file and the
    library calls are what they are without them.
"""
import argparse
import json
import time
from collections import Counter
from types import SimpleNamespace

import numpy as np

from . import coco_eval

CHUNK_WORDS = coco_eval.CHUNK_WORDS
CHUNK_IMAGES = coco_eval.CHUNK_IMAGES
LIB_CALLS = Counter()          # "s2d_selftrain_keep_ragged" and "chunks"; the decode calls are rle_ragged.LIB_CALLS, the IoU coco_eval.LIB_CALLS
FG_CATEGORIES = [{"id": 1, "name": "fg", "supercategory": "fg"}]


def keep_rule(inter, area_d, area_g):
    """the integer keep rule on numpy arrays: inter [D, G], area_d [D], area_g [G] -> bool [D], True where every g has
    2 * inter < area_d + area_g - inter (all True for G == 0)"""
    i = np.asarray(inter, np.int64).reshape(len(area_d), len(area_g))
    u = np.asarray(area_d, np.int64)[:, None] + np.asarray(area_g, np.int64)[None, :] - i
    return (2 * i < u).all(axis=1)


def device_keep(chunk, device=None, seconds=None):
    """the device side of one chunk (SimpleNamespace: segs per image = its D segmentations then its G ones, sizes, Ds, Gs, names) ->
    (keep int32 [sum Ds], boxes int32 [P, 4]) as numpy arrays; seconds: a dict that collects device-inclusive phase times"""
    import torch
    from . import ops
    from .rle_ragged import decode_ragged, stage_rle_ragged
    dev = coco_eval._device(device)

    def tick(name, t0):
        if seconds is not None:
            torch.cuda.synchronize(dev)
            seconds[name] = seconds.get(name, 0.0) + time.perf_counter() - t0
        return time.perf_counter()

    t0 = time.perf_counter()
    staged = stage_rle_ragged(chunk.segs, chunk.sizes, names=chunk.names)
    P, nd = staged.P, int(sum(chunk.Ds))
    t0 = tick("stage", t0)
    out = torch.empty((4 * P + nd,), device=dev, dtype=torch.int32)       # boxes, then keep flags: one read-back
    dec = decode_ragged(staged, dev, bbox_out=out[:4 * P].view(P, 4))
    t0 = tick("decode", t0)
    st = coco_eval.staged_chunk(dec.bits, chunk.Ds, chunk.Gs, chunk.sizes, np.zeros(int(sum(chunk.Gs)), np.uint8), dev)
    if st.words != staged.words:
        raise RuntimeError(f"chunk tables of {st.words} words for a buffer of {staged.words}")
    r = coco_eval.mask_iou_staged(st)
    t0 = tick("iou", t0)
    from ._lib import lib
    LIB_CALLS["s2d_selftrain_keep_ragged"] += 1
    lib().call("s2d_selftrain_keep_ragged", r.inter if r.inter.numel() else None, r.area_d if nd else None,
               r.area_g if r.area_g.numel() else None, st.img_dev, st.N, out[4 * P:] if nd else None, ops._stream())
    host = out.cpu().numpy()
    tick("keep", t0)
    return host[4 * P:], host[:4 * P].reshape(P, 4)


def _group(entries, images, what):
    by = {}
    for e in entries:
        iid = e["image_id"]
        if iid not in images:
            raise ValueError(f"image {iid}: {what} for an image the previous file's `images` does not have")
        by.setdefault(iid, []).append(e)
    return by


def _check_seg(e, im, what):
    seg = e.get("segmentation")
    if isinstance(seg, dict):
        if "counts" not in seg or [int(v) for v in seg.get("size", [])] != [im["height"], im["width"]]:
            raise ValueError(f"image {im['id']}: {what} with an RLE of size {seg.get('size')} in an image of size "
                             f"{[im['height'], im['width']]}")
    elif not isinstance(seg, (list, tuple)) or not seg:
        raise ValueError(f"image {im['id']}: {what} without a segmentation")
    return seg


def plan_round(prev_doc, predictions, threshold=0.7):
    """-> the per-image work items in output order (images with previous annotations, then images with predictions only), each a
    SimpleNamespace(iid, H, W, prev, pred: the entries; dsegs, gsegs: the segmentations to decode, empty where nothing needs them;
    keep, dbox, gbox: filled by merge_round)"""
    images = {im["id"]: im for im in prev_doc["images"]}
    pred = _group([p for p in predictions if p["score"] >= threshold], images, "a prediction")
    prev = _group(prev_doc["annotations"], images, "an annotation")
    items = []
    for iid in list(prev) + [k for k in pred if k not in prev]:
        im = images[iid]
        a, p = prev.get(iid, []), pred.get(iid, [])
        dsegs = [_check_seg(e, im, "an annotation") for e in a]
        gsegs = [_check_seg(e, im, "a prediction") for e in p]
        both = bool(a) and bool(p)
        items.append(SimpleNamespace(iid=iid, H=im["height"], W=im["width"], prev=a, pred=p,
                                     dsegs=dsegs if both or any(e.get("bbox") is None for e in a) else [],
                                     gsegs=gsegs if both or any(e.get("bbox") is None for e in p) else [],
                                     keep=[True] * len(a), dbox=None, gbox=None))
    return items


def _chunks(items):
    chunk, words = [], 0
    for it in items:
        n = len(it.dsegs) + len(it.gsegs)
        if not n:
            continue
        w = n * ((it.H * it.W + 31) // 32)
        if chunk and (words + w > CHUNK_WORDS or len(chunk) >= CHUNK_IMAGES):
            yield chunk
            chunk, words = [], 0
        chunk.append(it)
        words += w
    if chunk:
        yield chunk


def merge_round(prev_doc, predictions, threshold=0.7, device=None, keep_fn=None, seconds=None):
    """loaded documents -> the next round's annotation document (module docstring).  keep_fn: (chunk) -> (keep flags [sum Ds], boxes
    [P, 4]) replaces the device side (device_keep), so the host logic runs without a device; seconds: a dict that collects the phase
    times (stage, decode, iou, keep: device-inclusive; assemble)."""
    if keep_fn is None:
        keep_fn = lambda chunk: device_keep(chunk, device, seconds)      # noqa: E731
    t0 = time.perf_counter()
    items = plan_round(prev_doc, predictions, threshold)
    host = time.perf_counter() - t0
    for part in _chunks(items):
        chunk = SimpleNamespace(items=part, segs=[it.dsegs + it.gsegs for it in part], sizes=[(it.H, it.W) for it in part],
                                Ds=[len(it.dsegs) for it in part], Gs=[len(it.gsegs) for it in part], names=[it.iid for it in part])
        LIB_CALLS["chunks"] += 1
        keep, boxes = keep_fn(chunk)
        keep, boxes = np.asarray(keep).reshape(-1), np.asarray(boxes).reshape(-1, 4)
        if len(keep) != sum(chunk.Ds) or len(boxes) != sum(chunk.Ds) + sum(chunk.Gs):
            raise ValueError(f"keep_fn returned {len(keep)} flags and {len(boxes)} boxes for a chunk of {sum(chunk.Ds)} + {sum(chunk.Gs)}")
        t0 = time.perf_counter()
        d0 = p0 = 0
        for it, D, G in zip(part, chunk.Ds, chunk.Gs):
            if D:
                it.dbox = boxes[p0:p0 + D].tolist()
                if G:
                    it.keep = [bool(k) for k in keep[d0:d0 + D]]
            if G:
                it.gbox = boxes[p0 + D:p0 + D + G].tolist()
            d0, p0 = d0 + D, p0 + D + G
        host += time.perf_counter() - t0
    t0 = time.perf_counter()
    out = {k: prev_doc[k] for k in ("info", "licenses") if k in prev_doc}
    out["categories"] = prev_doc["categories"] if prev_doc.get("categories") else [dict(c) for c in FG_CATEGORIES]
    cats = {c["id"] for c in out["categories"]}
    merged = []

    def emit(it, e, box):
        a = dict(e)
        if a.get("bbox") is None:
            a["bbox"] = [float(v) for v in box]
        if a.get("category_id") not in cats:
            raise ValueError(f"image {it.iid}: category_id {a.get('category_id')!r} is not among the output categories {sorted(cats)}")
        seg = a["segmentation"]
        size = seg["size"] if isinstance(seg, dict) else [it.H, it.W]
        a["id"] = len(merged) + 1
        a["area"] = a["bbox"][-1] * a["bbox"][-2]
        a["iscrowd"] = 0
        a["width"], a["height"] = size[0], size[1]                       # swapped, as the reference writes them
        merged.append(a)

    for it in items:
        for k, e in enumerate(it.pred):
            emit(it, e, it.gbox[k] if it.gbox else None)
        for k, e in enumerate(it.prev):
            if it.keep[k]:
                emit(it, e, it.dbox[k] if it.dbox else None)
    out["images"] = prev_doc["images"]
    out["annotations"] = merged
    if seconds is not None:
        seconds["assemble"] = seconds.get("assemble", 0.0) + host + time.perf_counter() - t0
    return out


def merge_files(new_pred, prev_ann, save_path, threshold=0.7, device=None, keep_fn=None, seconds=None, cleanup=None):
    """the command line on paths -> the written document.  cleanup: a clean_annotations.cleanup_options dict; when it asks for
    anything the merged document's masks are cleaned just before it is written (area = bbox w * h, as every annotation here)"""
    t0 = time.perf_counter()
    with open(new_pred) as fh:
        predictions = json.load(fh)
    with open(prev_ann) as fh:
        prev_doc = json.load(fh)
    t_json = time.perf_counter() - t0
    doc = merge_round(prev_doc, predictions, threshold, device=device, keep_fn=keep_fn, seconds=seconds)
    if cleanup:
        from .clean_annotations import clean_merged
        doc = clean_merged(doc, cleanup, area_rule="bbox", device=device)
    t0 = time.perf_counter()
    with open(save_path, "w") as fh:
        json.dump(doc, fh)
    if seconds is not None:
        seconds["json"] = seconds.get("json", 0.0) + t_json + time.perf_counter() - t0
    return doc


def main(argv=None):
    ap = argparse.ArgumentParser(description="Generate json files for the self-training")
    ap.add_argument("--new-pred", type=str, default="output/inference/coco_instances_results.json", help="Path to model predictions")
    ap.add_argument("--prev-ann", type=str, default="DETECTRON2_DATASETS/imagenet/annotations/cutler_imagenet1k_train.json",
                    help="Path to annotations in the previous round")
    ap.add_argument("--save-path", type=str, default="DETECTRON2_DATASETS/imagenet/annotations/cutler_imagenet1k_train_r1.json",
                    help="Path to save the generated annotation file")
    ap.add_argument("--threshold", type=float, default=0.7, help="Confidence score thresholds")
    from .clean_annotations import add_cleanup_arguments, cleanup_options
    a = add_cleanup_arguments(ap).parse_args(argv)
    doc = merge_files(a.new_pred, a.prev_ann, a.save_path, a.threshold, cleanup=cleanup_options(a))
    print("Done: {} images; {} anns.".format(len(doc["images"]), len(doc["annotations"])))


if __name__ == "__main__":
    main()
