"""Training on COCO-format image annotations as pseudo-clips: the reference's CocoClipDatasetMapper (data_video/
dataset_mapper.py:593-704; what configs/imagenet_video/video_mask2former_R50_cls_agnostic.yaml trains on) without detectron2
and without pycocotools, with the masks made and warped on the device.

One image becomes a SAMPLING_FRAME_NUM-frame clip: the augmentation is drawn T times (ClipAugmentation.sample: size and flip
once per clip, the rest per frame) and applied to the same image.  Every non-crowd annotation is one instance whose id is its
index among them, so a "track" is one object under T transforms: slot s is the s-th non-crowd annotation at every frame.

Per clip the image is decoded on the host and uploaded once; on the device it is replicated and warped by
s2d_aug_warp_frames_hwc_u8; RLE instances are parsed and decoded to bit planes (ytvis_eval.stage_rle / decode_staged), polygon
instances are rasterised into the same [S, ceil(H*W/32)] tensor by one s2d_polygons_to_bits call, and s2d_aug_warp_mask_bits warps
all of them and counts their pixels (`gt_ids = -1` where the count is 0, as in train_loader._finish_clip).

Polygon fill rule (the library's own): pixel (x, y) is set iff its centre (x + 0.5, y + 0.5) is inside at least one of the
instance's polygons by the even-odd rule.  pycocotools' frPoly walks a 5x-upsampled boundary instead, so masks can differ from it
at boundary pixels: parity unpinned."""
import json
import os

import numpy as np
import torch

from .augment import augment_frames_hwc, warp_mask_bits
from .test_loader import read_frame
from .train_loader import YTVISTrainLoader, _device


# ------------------------------------------------------------------------------------------------------------------ dataset
def detect_train_format(doc):
    """"coco_image" for a document with `images` and no `videos`, else "ytvis" """
    return "coco_image" if "images" in doc and "videos" not in doc else "ytvis"


def _valid_polygons(seg):
    """the polygons of a COCO segmentation list that can be filled: an even number of coordinates, at least 3 vertices"""
    out = []
    for poly in seg:
        if isinstance(poly, (list, tuple)) and len(poly) >= 6 and len(poly) % 2 == 0:
            out.append([float(v) for v in poly])
    return out


def load_coco_image_train(json_file, image_root, filter_empty=True):
    """one record per image (sorted by id): {"file_name", "height", "width", "image_id", "annotations": [{"id", "category_id"
    (contiguous, sorted order), "iscrowd", "segmentation"}]}.  A segmentation is an RLE dict (compressed or uncompressed; its
    size must be the image's) or a list of polygons [x0, y0, x1, y1, ...]; a polygon with an odd number of coordinates or fewer
    than 6 is dropped, an annotation left without a segmentation is skipped.  filter_empty: drop images without a non-crowd
    annotation (DATALOADER.FILTER_EMPTY_ANNOTATIONS)."""
    doc = json.load(open(json_file)) if isinstance(json_file, str) else json_file
    cat_ids = sorted(c["id"] for c in doc.get("categories", []))
    id_map = {v: i for i, v in enumerate(cat_ids)}
    by_img = {}
    for a in doc.get("annotations", []):
        by_img.setdefault(a["image_id"], []).append(a)
    out = []
    for im in sorted(doc["images"], key=lambda im: im["id"]):
        iid, H, W = im["id"], im["height"], im["width"]
        objs = []
        for a in by_img.get(iid, []):
            seg = a.get("segmentation")
            if isinstance(seg, dict):
                if [int(s) for s in seg["size"]] != [H, W]:
                    raise ValueError(f"image {iid}: RLE of size {seg['size']} in an image of size {[H, W]}")
            elif isinstance(seg, (list, tuple)):
                seg = _valid_polygons(seg)
                if not seg:
                    continue
            else:
                continue
            objs.append({"id": a["id"], "category_id": id_map[a["category_id"]] if id_map else a["category_id"],
                         "iscrowd": int(a.get("iscrowd", 0)), "segmentation": seg})
        out.append({"file_name": os.path.join(image_root, im["file_name"]), "height": H, "width": W, "image_id": iid,
                    "annotations": objs})
    if filter_empty:
        out = [r for r in out if any(o["iscrowd"] == 0 for o in r["annotations"])]
    return out


# ------------------------------------------------------------------------------------------------------------------ polygons
def stage_polygons(planes):
    """planes: per plane a list of polygons, each flat [x0, y0, x1, y1, ...] or [n, 2] -> (verts float32 [V, 2], poly_off int32
    [NP+1], plane_off int32 [P+1]), the inputs of s2d_polygons_to_bits"""
    polys = [np.asarray(p, np.float32).reshape(-1, 2) for pl in planes for p in pl]
    poly_off = np.zeros(len(polys) + 1, np.int32)
    np.cumsum([len(p) for p in polys], out=poly_off[1:])
    plane_off = np.zeros(len(planes) + 1, np.int32)
    np.cumsum([len(pl) for pl in planes], out=plane_off[1:])
    verts = np.concatenate(polys) if polys else np.zeros((0, 2), np.float32)
    return np.ascontiguousarray(verts), poly_off, plane_off


def polygons_to_bits(planes, H, W, device=None, out=None, rows=None, pinned=False):
    """per plane a list of polygons (source-pixel coordinates, any values) -> int32 CUDA bit planes [P, ceil(H*W/32)] in the
    layout of ytvis_eval.decode_frames, on the current stream (s2d_polygons_to_bits; the fill rule is in the module docstring).
    out, rows: write plane p into row rows[p] of `out` [R, ceil(H*W/32)] instead (distinct rows; the other rows are not touched).
    pinned: the tables go up from pinned memory without blocking the host (a loader's side stream)."""
    from .._lib import lib
    from .augment import _stream
    dev = out.device if out is not None else _device(device)
    wpp = (H * W + 31) // 32
    P = len(planes)
    if out is None:
        if rows is not None:
            raise ValueError("rows needs out")
        out = torch.empty((P, wpp), device=dev, dtype=torch.int32)
    elif out.dtype != torch.int32 or out.dim() != 2 or out.shape[1] != wpp or not out.is_contiguous():
        raise ValueError("out must be contiguous int32 [R, ceil(H*W/32)]")
    if rows is not None:
        rows = np.ascontiguousarray(rows, np.int32)
        if rows.shape != (P,) or len(set(rows.tolist())) != P or (P and (rows.min() < 0 or rows.max() >= out.shape[0])):
            raise ValueError(f"rows must be {P} distinct rows of out")
    elif out.shape[0] < P:
        raise ValueError(f"out has {out.shape[0]} rows for {P} planes")
    if P == 0:
        return out
    verts, poly_off, plane_off = stage_polygons(planes)
    up = (lambda a: torch.from_numpy(a).pin_memory().to(dev, non_blocking=True)) if pinned else (lambda a: torch.from_numpy(a).to(dev))
    verts_d = up(verts) if len(verts) else None
    rows_d = up(rows) if rows is not None else None
    lib().call("s2d_polygons_to_bits", verts_d, len(verts), up(poly_off), poly_off, len(poly_off) - 1, up(plane_off), plane_off, P,
               rows_d, out.shape[0], H, W, out, _stream())
    return out


# ------------------------------------------------------------------------------------------------------------------ the mapper
def plan_image_clip(record, py_rng, np_rng, st):
    """host half of the mapper: the T augmentation draws, the slots (slot s = the s-th non-crowd annotation at every frame, its
    plane is s) and the split of the instances into RLE and polygon planes.  There is no frame selection; py_rng is unused."""
    T, H0, W0 = st.num_frames, record["height"], record["width"]
    params, out_hw = st.aug.sample(T, H0, W0, rng=np_rng)
    objs = [a for a in record["annotations"] if a.get("iscrowd", 0) == 0]
    S = len(objs)
    plane_of = np.tile(np.arange(S, dtype=np.int32), (T, 1))
    gt_ids = np.tile(np.arange(S, dtype=np.int64), (T, 1))
    classes = np.tile(np.asarray([a["category_id"] for a in objs], np.int64).reshape(1, S), (T, 1))
    rle = [a["segmentation"] if isinstance(a["segmentation"], dict) else None for a in objs]     # None: an all-zero plane
    poly_slots = [s for s, a in enumerate(objs) if not isinstance(a["segmentation"], dict)]
    return {"record": record, "params": params, "out_hw": out_hw, "plane_of": plane_of, "gt_ids": gt_ids, "gt_classes": classes,
            "rle": rle, "poly_slots": poly_slots, "polys": [objs[s]["segmentation"] for s in poly_slots]}


def _read_image(plan, pool, fmt):
    """a future (or the array, without a pool) of the image, decoded as read_image decodes it"""
    name = plan["record"]["file_name"]
    return pool.submit(read_frame, name, fmt) if pool is not None else read_frame(name, fmt)


def _stage_image(plan, image):
    """the decoded image (array or future) -> a pinned [1][H0][W0][3] buffer"""
    rec = plan["record"]
    H0, W0 = rec["height"], rec["width"]
    a = image.result() if hasattr(image, "result") else image
    if a.shape[:2] != (H0, W0):
        raise ValueError(f"image {rec['image_id']}: {rec['file_name']} is {a.shape[:2]}, the record says {(H0, W0)}")
    buf = torch.empty((1, H0, W0, 3), dtype=torch.uint8, pin_memory=True)
    buf[0].numpy()[...] = a
    return buf


def image_clip_bits(plan, device, pinned=False):
    """the instances of a plan -> int32 CUDA bit planes [S, ceil(H0*W0/32)] in slot order: the RLE instances decoded, then the
    polygon instances rasterised into their rows of the same tensor"""
    from ..ytvis_eval import decode_staged, stage_rle
    rec = plan["record"]
    H0, W0 = rec["height"], rec["width"]
    bits = decode_staged(stage_rle(plan["rle"], H0, W0), H0, W0, device, pinned=pinned)
    if plan["poly_slots"]:
        polygons_to_bits(plan["polys"], H0, W0, out=bits, rows=plan["poly_slots"], pinned=pinned)
    return bits


def _launch_image_clip(plan, image_pinned, device):
    """device half on the current stream: the image and the annotation tables go up non-blocking from pinned memory, then
    replicate, warp, decode / rasterise, warp, count"""
    rec = plan["record"]
    H0, W0 = rec["height"], rec["width"]
    T = len(plan["params"])
    x = image_pinned.to(device, non_blocking=True).expand(T, H0, W0, 3).contiguous()
    p = torch.from_numpy(np.ascontiguousarray(plan["params"], np.float32)).pin_memory().to(device, non_blocking=True)
    img = augment_frames_hwc(x, p, plan["out_hw"])
    bits = image_clip_bits(plan, device, pinned=True)
    masks, area = warp_mask_bits(bits, plan["plane_of"], H0, W0, p, plan["out_hw"])
    area_h = torch.empty(area.shape, dtype=torch.int32, pin_memory=True)
    area_h.copy_(area, non_blocking=True)
    return img, masks, area_h


def _finish_image_clip(plan, img, masks, area_h):
    """filter_empty_instances on the counts (call after the stream that produced area_h has been synchronised)"""
    rec = plan["record"]
    gt_ids = plan["gt_ids"].copy()
    gt_ids[area_h.numpy() == 0] = -1
    mb = masks.view(torch.bool)
    T = img.shape[0]
    inst = [{"gt_masks": mb[t], "gt_ids": gt_ids[t].copy(), "gt_classes": plan["gt_classes"][t].copy()} for t in range(T)]
    return {"image": [img[t] for t in range(T)], "instances": inst, "height": rec["height"], "width": rec["width"], "length": T,
            "video_id": rec["image_id"], "image_id": rec["image_id"], "file_names": [rec["file_name"]] * T}


def map_image_clip(record, py_rng, np_rng, settings, device=None, pool=None):
    """the image-to-clip mapper on one record, synchronously on the current stream: -> the dict layout of train_loader.map_clip
    (`file_names` holds the image's name T times, `length` is T, `video_id` is the image id)"""
    device = _device(device)
    plan = plan_image_clip(record, py_rng, np_rng, settings)
    buf = _stage_image(plan, _read_image(plan, pool, settings.fmt))
    img, masks, area_h = _launch_image_clip(plan, buf, device)
    torch.cuda.current_stream(device).synchronize()
    return _finish_image_clip(plan, img, masks, area_h)


# ------------------------------------------------------------------------------------------------------------------ the loader
class COCOImageTrainLoader(YTVISTrainLoader):
    """YTVISTrainLoader (sampler, aspect grouping, prefetch thread, side stream, resume) over load_coco_image_train records"""
    _plan, _read, _stage = staticmethod(plan_image_clip), staticmethod(_read_image), staticmethod(_stage_image)
    _launch, _finish = staticmethod(_launch_image_clip), staticmethod(_finish_image_clip)
