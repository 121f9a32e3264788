"""Helpers of the self-training merge tests: a numpy restatement of the tool (written from its behaviour list, masks as dense
arrays, the keep rule as the reference's float32 `inter / union < 0.5`), a numpy keep_fn for merge_round, and case builders."""
import numpy as np

from oracle import oracle_np

SIZES = [(1, 1), (1, 33), (37, 1), (2, 31), (3, 32), (5, 63), (5, 64), (7, 65), (4, 255), (3, 256), (2, 257), (37, 300)]


# ------------------------------------------------------------------------------------------------------------------ masks
def counts_of(mask):
    """uncompressed COCO RLE counts of a [H, W] 0/1 mask (column-major runs, zeros first)"""
    flat = (np.asarray(mask) != 0).T.reshape(-1).astype(np.int8)
    edges = np.flatnonzero(np.diff(flat)) + 1
    counts = np.diff(np.concatenate([[0], edges, [len(flat)]])).tolist()
    return ([0] if flat[0] else []) + counts


def compress(counts):
    """maskApi.c rleToString of a counts list -> str"""
    s = bytearray()
    for i, x in enumerate(counts):
        x = int(x)
        if i > 2:
            x -= int(counts[i - 2])
        more = True
        while more:
            ch = x & 0x1F
            x >>= 5
            more = (x != -1) if (ch & 0x10) else (x != 0)
            if more:
                ch |= 0x20
            s.append(ch + 48)
    return s.decode()


def rle_u(mask):
    return {"size": [int(mask.shape[0]), int(mask.shape[1])], "counts": counts_of(mask)}


def rle_c(mask):
    return {"size": [int(mask.shape[0]), int(mask.shape[1])], "counts": compress(counts_of(mask))}


def fill_polygons(polys, H, W):
    """pixel (x, y) is set iff its centre is inside at least one polygon by the even-odd rule; float64.  The tests use axis-aligned
    edges on integer coordinates, so no centre lies on an edge and the rule leaves nothing to rounding"""
    ys, xs = np.mgrid[0:H, 0:W]
    px, py = xs + 0.5, ys + 0.5
    out = np.zeros((H, W), bool)
    for poly in polys:
        v = np.asarray(poly, np.float64).reshape(-1, 2)
        inside = np.zeros((H, W), bool)
        for (x0, y0), (x1, y1) in zip(v, np.roll(v, -1, 0)):
            if y0 == y1:
                continue
            cross = ((y0 <= py) != (y1 <= py)) & (px < x0 + (py - y0) * (x1 - x0) / (y1 - y0))
            inside ^= cross
        out |= inside
    return out


def seg_mask(seg, H, W):
    """a COCO segmentation -> bool [H, W]; None -> all zero.  RLE through oracle_np.rle_decode (runs past H*W are cut)"""
    if seg is None:
        return np.zeros((H, W), bool)
    if isinstance(seg, (list, tuple)):
        return fill_polygons(seg, H, W)
    assert list(seg["size"]) == [H, W]
    c = seg["counts"]
    if isinstance(c, (list, tuple)):
        c = compress(c)
    return oracle_np.rle_decode({"size": [H, W], "counts": c}).astype(bool)


def pack_bits(mask):
    """bool [H, W] -> uint32 words of the flat row-major plane (pixel i -> word i/32, bit i%32, tail bits zero)"""
    flat = np.asarray(mask, bool).reshape(-1)
    pad = np.zeros((len(flat) + 31) // 32 * 32, np.uint8)
    pad[:len(flat)] = flat
    return (pad.reshape(-1, 32).astype(np.uint32) << np.arange(32, dtype=np.uint32)).sum(1, dtype=np.uint64).astype(np.uint32)


def box_of(mask):
    return [int(v) for v in oracle_np.rle_area_bbox(mask)[1]]


def f32_keep(inter, area_d, area_g):
    """the reference's rule: iou_max < 0.5 on float32 inter / union (NaN compares false); True for no prediction"""
    i = np.asarray(inter, np.int64).reshape(len(area_d), len(area_g))
    u = np.asarray(area_d, np.int64)[:, None] + np.asarray(area_g, np.int64)[None, :] - i
    with np.errstate(invalid="ignore", divide="ignore"):
        iou = i.astype(np.float32) / u.astype(np.float32)
    if iou.shape[1] == 0:
        return np.ones(len(area_d), bool)
    return iou.max(axis=1) < np.float32(0.5)                              # max propagates NaN, and NaN < 0.5 is False


def numpy_keep(chunk):
    """merge_round's keep_fn on the host: (keep [sum Ds], boxes [P, 4])"""
    keep, boxes = [], []
    for segs, (H, W), D, G in zip(chunk.segs, chunk.sizes, chunk.Ds, chunk.Gs):
        masks = [seg_mask(s, H, W) for s in segs]
        boxes += [box_of(m) for m in masks]
        d, g = masks[:D], masks[D:]
        inter = np.array([[int((a & b).sum()) for b in g] for a in d], np.int64).reshape(D, G)
        keep += f32_keep(inter, [int(a.sum()) for a in d], [int(b.sum()) for b in g]).tolist()
    return np.array(keep, np.int32), np.array(boxes, np.int32).reshape(-1, 4)


# ------------------------------------------------------------------------------------------------------------------ the tool
def reference_merge(prev_doc, predictions, threshold=0.7):
    """the tool restated on dense masks, image by image"""
    size = {im["id"]: (im["height"], im["width"]) for im in prev_doc["images"]}
    pred, prev = {}, {}
    for p in predictions:
        if p["score"] >= threshold:
            pred.setdefault(p["image_id"], []).append(p)
    for a in prev_doc["annotations"]:
        prev.setdefault(a["image_id"], []).append(a)
    merged = []
    for iid, anns in prev.items():
        H, W = size[iid]
        if iid not in pred:
            merged += [(a, iid) for a in anns]
            continue
        d = [seg_mask(a["segmentation"], H, W) for a in anns]
        g = [seg_mask(p["segmentation"], H, W) for p in pred[iid]]
        inter = np.array([[int((a & b).sum()) for b in g] for a in d], np.int64)
        keep = f32_keep(inter, [int(a.sum()) for a in d], [int(b.sum()) for b in g])
        merged += [(p, iid) for p in pred[iid]] + [(a, iid) for a, k in zip(anns, keep) if k]
    for iid, ps in pred.items():
        if iid not in prev:
            merged += [(p, iid) for p in ps]
    out = []
    for n, (e, iid) in enumerate(merged):
        H, W = size[iid]
        a = dict(e)
        if a.get("bbox") is None:
            a["bbox"] = [float(v) for v in box_of(seg_mask(a["segmentation"], H, W))]
        a["id"], a["area"], a["iscrowd"] = n + 1, a["bbox"][2] * a["bbox"][3], 0
        a["width"], a["height"] = H, W                                    # the reference's swap: size[0] is the height
        out.append(a)
    doc = {k: prev_doc[k] for k in ("info", "licenses") if k in prev_doc}
    doc["categories"] = prev_doc.get("categories") or [{"id": 1, "name": "fg", "supercategory": "fg"}]
    doc["images"], doc["annotations"] = prev_doc["images"], out
    return doc


# ------------------------------------------------------------------------------------------------------------------ cases
def pair(H, W, inter, area_d, area_g):
    """two masks of an H x W image with exactly these counts: d = flat pixels [0, area_d), g = [area_d - inter, .. + area_g)"""
    assert inter <= min(area_d, area_g) and area_d - inter + area_g <= H * W
    d, g = np.zeros(H * W, bool), np.zeros(H * W, bool)
    d[:area_d] = True
    g[area_d - inter:area_d - inter + area_g] = True
    return d.reshape(H, W), g.reshape(H, W)


# name -> (inter, area_d, area_g, kept): IoU exactly one half is not kept, just below is; two empty masks: dropped
NAMED_PAIRS = {"half": (2, 3, 3, False), "below": (2, 3, 4, True), "near_below": (499, 750, 749, True), "near_half": (500, 750, 750, False),
               "above": (3, 4, 4, False), "disjoint": (0, 5, 7, True), "empty_both": (0, 0, 0, False), "empty_prev": (0, 0, 9, True)}


def blob(H, W, rng):
    """a random box or ellipse, at least one pixel"""
    y0, x0 = int(rng.integers(0, H)), int(rng.integers(0, W))
    y1, x1 = int(rng.integers(y0, H)) + 1, int(rng.integers(x0, W)) + 1
    m = np.zeros((H, W), bool)
    m[y0:y1, x0:x1] = True
    if rng.random() < 0.5 and y1 - y0 > 2 and x1 - x0 > 2:
        ys, xs = np.mgrid[0:H, 0:W]
        m &= ((ys - (y0 + y1 - 1) / 2) / ((y1 - y0) / 2)) ** 2 + ((xs - (x0 + x1 - 1) / 2) / ((x1 - x0) / 2)) ** 2 <= 1.0
        m[y0, x0] = True
    return m


def jitter(m, rng):
    """m shifted by up to 2 pixels: a prediction that overlaps its pseudo mask"""
    return np.roll(m, (int(rng.integers(-2, 3)), int(rng.integers(-2, 3))), (0, 1))


def named_case():
    """hand-built documents: one image per named pair (4 x 255), an image with previous annotations only, one with predictions
    only, one with both kinds and several of each, scores at, above and below the threshold, entries with and without bbox"""
    H, W = 4, 255
    images, anns, preds = [], [], []
    for k, (name, (i, ad, ag, _)) in enumerate(NAMED_PAIRS.items()):
        iid = 10 + k
        images.append({"id": iid, "height": H, "width": W, "file_name": f"{name}.jpg"})
        d, g = pair(H, W, i, ad, ag)
        anns.append({"id": 100 + k, "image_id": iid, "category_id": 1, "segmentation": rle_c(d), "bbox": [0, 0, 1, 1], "area": 1, "iscrowd": 0})
        preds.append({"image_id": iid, "category_id": 1, "score": 0.7 if k % 2 else 0.93, "segmentation": rle_u(g) if k % 3 == 0 else rle_c(g)})
    rng = np.random.default_rng(5)
    images += [{"id": 3, "height": 37, "width": 300, "file_name": "prev_only.jpg"}, {"id": 2, "height": 5, "width": 63, "file_name": "pred_only.jpg"},
               {"id": 7, "height": 37, "width": 300, "file_name": "both.jpg"}, {"id": 8, "height": 7, "width": 65, "file_name": "low_scores.jpg"},
               {"id": 9, "height": 2, "width": 31, "file_name": "unused.jpg"}]
    a = [blob(37, 300, rng) for _ in range(3)]
    anns += [{"id": 300 + j, "image_id": 3, "category_id": 1, "segmentation": rle_c(m), **({"bbox": [1.0, 2.0, 3.0, 4.0]} if j else {})}
             for j, m in enumerate(a)]
    preds += [{"image_id": 2, "category_id": 1, "score": 0.8, "segmentation": rle_c(blob(5, 63, rng)), "bbox": [0.0, 0.0, 2.0, 2.0]},
              {"image_id": 2, "category_id": 1, "score": 0.71, "segmentation": rle_c(blob(5, 63, rng))}]
    b = [blob(37, 300, rng) for _ in range(4)]
    anns += [{"id": 400 + j, "image_id": 7, "category_id": 1, "segmentation": rle_u(m) if j == 1 else rle_c(m)} for j, m in enumerate(b)]
    preds += [{"image_id": 7, "category_id": 1, "score": 0.9, "segmentation": rle_c(b[0])},                    # the same mask: IoU 1
              {"image_id": 7, "category_id": 1, "score": 0.69999, "segmentation": rle_c(b[1])},                # below the threshold
              {"image_id": 7, "category_id": 1, "score": 0.75, "segmentation": rle_u(b[2]), "bbox": [5, 5, 5, 5]}]
    anns.append({"id": 500, "image_id": 8, "category_id": 1, "segmentation": rle_c(blob(7, 65, rng)), "bbox": [0, 0, 3, 2]})
    preds.append({"image_id": 8, "category_id": 1, "score": 0.1, "segmentation": rle_c(blob(7, 65, rng))})     # not kept: as prev only
    # file order differs from image order: the previous annotations of image 7 come first
    anns = [x for x in anns if x["image_id"] == 7] + [x for x in anns if x["image_id"] != 7]
    doc = {"info": {"description": "round 0"}, "images": images, "annotations": anns,
           "categories": [{"id": 1, "name": "fg", "supercategory": "fg"}]}
    return doc, preds


def random_case(n_images=40, seed=0):
    """about n_images synthetic images: sizes from SIZES plus 120 x 160, 0-4 previous masks and 0-6 predictions each (no bbox), one
    image with polygon pseudo masks (integer vertices)"""
    rng = np.random.default_rng(seed)
    sizes = [SIZES[k % len(SIZES)] if k % 5 else (120, 160) for k in range(n_images)]
    images, anns, preds = [], [], []
    for k, (H, W) in enumerate(sizes):
        iid = 1000 + (k * 7) % n_images if n_images % 7 else 1000 + k
        images.append({"id": iid, "height": H, "width": W, "file_name": f"{iid}.jpg"})
        masks = [blob(H, W, rng) for _ in range(int(rng.integers(0, 5)))]
        for j, m in enumerate(masks):
            anns.append({"id": len(anns) + 1, "image_id": iid, "category_id": 1, "iscrowd": 0,
                         "segmentation": rle_u(m) if (k + j) % 3 == 0 else rle_c(m)})
        for j in range(int(rng.integers(0, 7))):
            m = jitter(masks[j % len(masks)], rng) if masks and rng.random() < 0.6 else blob(H, W, rng)
            preds.append({"image_id": iid, "category_id": 1, "score": float(np.round(rng.uniform(0.5, 1.0), 3)), "segmentation": rle_c(m)})
    iid = 5000
    images.append({"id": iid, "height": 120, "width": 160, "file_name": "poly.jpg"})
    polys = [[[10, 10, 60, 10, 60, 50, 10, 50]], [[80, 20, 150, 20, 150, 60, 120, 60, 120, 100, 80, 100], [5, 60, 30, 60, 30, 110, 5, 110]], [[100, 5, 140, 5, 140, 15, 100, 15]]]
    anns += [{"id": len(anns) + 1 + j, "image_id": iid, "category_id": 1, "iscrowd": 0, "segmentation": p} for j, p in enumerate(polys)]
    preds.append({"image_id": iid, "category_id": 1, "score": 0.9, "segmentation": rle_c(fill_polygons(polys[0], 120, 160))})
    preds.append({"image_id": iid, "category_id": 1, "score": 0.8, "segmentation": rle_c(blob(120, 160, rng))})
    order = rng.permutation(len(preds))
    return {"images": images, "annotations": anns, "categories": [{"id": 1, "name": "fg", "supercategory": "fg"}]}, [preds[i] for i in order]
