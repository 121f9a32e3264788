"""Host references of the ragged bit-plane morphology (s2d_amd/plane_morph.py) and of the annotation cleanup with smoothing
(s2d_amd/clean_annotations.py), with the constructed cases of their tests.  None of them restates the kernel: the primitives are
scipy.ndimage.binary_erosion / binary_dilation with the border values of the rule, checked against a brute-force double loop of the
definitions, and the document reference is tests/plane_components_refs.py's applied to the smoothed planes.

The rule (s2d_amd/plane_morph.py): B(r, disk) = {dx^2 + dy^2 <= r^2}, B(r, square) = {|dx|, |dy| <= r}; dilate has a zero border,
erode counts pixels outside the image as set; open = dilate(erode(.)), close = erode(dilate(.)); cleanup = fill(filter(close(open(.))))."""
import numpy as np
from scipy import ndimage

from tests import plane_components_refs as C

OPS = ("erode", "dilate", "open", "close")
SHAPES = ("disk", "square")


# ---------------------------------------------------------------------------------------------------------------- the primitives
def disk(r):
    yy, xx = np.mgrid[-r:r + 1, -r:r + 1]
    return yy * yy + xx * xx <= r * r


def square(r):
    return np.ones((2 * r + 1, 2 * r + 1), bool)


def element(r, shape):
    if shape not in SHAPES:
        raise ValueError(f"shape {shape!r}")
    return disk(r) if shape == "disk" else square(r)


def _fit(B, H, W):
    """B without the offsets that cannot matter in an H x W image: |dy| >= H or |dx| >= W never joins two pixels of the image, so
    under either border value of the rule the result is the same, and scipy walks 5 x 129 offsets for a 3-row plane at r = 64
    instead of 129 x 129 (tests/test_plane_morph_refs_cpu.py holds the cut against the whole element)"""
    r = B.shape[0] // 2
    ry, rx = min(r, H - 1), min(r, W - 1)
    return B[r - ry:r + ry + 1, r - rx:r + rx + 1]


def erode(x, r, shape="disk", fit=True):
    x = np.asarray(x, bool)
    if r == 0 or (fit and x.all()):                                     # a full plane stays full: scipy would walk every offset of every pixel
        return x.copy()
    B = element(r, shape)
    return ndimage.binary_erosion(x, _fit(B, *x.shape) if fit else B, border_value=1)


def dilate(x, r, shape="disk", fit=True):
    x = np.asarray(x, bool)
    if r == 0 or (fit and not x.any()):                                 # an empty plane stays empty
        return x.copy()
    B = element(r, shape)
    return ndimage.binary_dilation(x, _fit(B, *x.shape) if fit else B, border_value=0)


def open_(x, r, shape="disk"):
    return dilate(erode(x, r, shape), r, shape)


def close(x, r, shape="disk"):
    return erode(dilate(x, r, shape), r, shape)


def morph(x, op, r, shape="disk"):
    return {"erode": erode, "dilate": dilate, "open": open_, "close": close}[op](x, r, shape)


def brute(x, op, r, shape="disk"):
    """the definitions by a double loop over the offsets (dy, dx) of B, each a shifted copy of the plane with the border value of the
    rule where p + (dy, dx) leaves the image: the check of the scipy restatements on tiny planes.  It costs one pass over the plane
    per offset, where scipy builds a table of pixels x offsets once the element is larger than the plane; so the GPU rows at r >= 31
    compare against this one (the CPU file holds the two equal there as well).  Offsets with |dy| >= H or |dx| >= W are skipped:
    they leave the image from every pixel, and there the border value is the neutral element"""
    x = np.asarray(x, bool)
    H, W = x.shape
    ry, rx = min(r, H - 1), min(r, W - 1)

    def one(src, er):
        pad = np.full((H + 2 * r, W + 2 * r), bool(er))                 # outside the image: set for erode, clear for dilate
        pad[r:r + H, r:r + W] = src
        out = np.full((H, W), bool(er))
        for dy in range(-ry, ry + 1):
            for dx in range(-rx, rx + 1):
                if shape == "disk" and dy * dy + dx * dx > r * r:
                    continue
                v = pad[r + dy:r + dy + H, r + dx:r + dx + W]
                out = (out & v) if er else (out | v)
        return out

    if op == "erode":
        return one(x, True)
    if op == "dilate":
        return one(x, False)
    return one(one(x, True), False) if op == "open" else one(one(x, False), True)


def smooth(x, open_r=0, close_r=0, shape="disk"):
    """close(open(x)), each skipped at radius 0"""
    return close(open_(x, open_r, shape), close_r, shape)


def ref_smooth_clean(mask, open_r=0, close_r=0, shape="disk", min_area=0, keep_largest=False, max_hole_area=0, conn=8):
    """plane_components_refs.ref_clean applied to close(open(mask)) -> (out, removed, filled, opened, closed): removed / filled count
    against the smoothed plane, opened / closed are the pixels of `mask` the smoothing cleared / set"""
    m = np.asarray(mask, bool)
    s = smooth(m, open_r, close_r, shape)
    o, removed, filled = C.ref_clean(s, min_area, keep_largest, max_hole_area, conn)
    return o, removed, filled, int((m & ~s).sum()), int((s & ~m).sum())


# ---------------------------------------------------------------------------------------------------------------- radii
def ref_radius(spec, H, W):
    """N, "N" or "X%" -> pixels: X percent of the image diagonal, rounded as Python rounds, at least 1 (the Boundary IoU band's rule)"""
    if isinstance(spec, str) and spec.strip().endswith("%"):
        x = float(spec.strip()[:-1])
        return max(1, int(round(x / 100.0 * np.sqrt(H * H + W * W)))) if x > 0 else 0
    return int(spec)


# ---------------------------------------------------------------------------------------------------------------- the document
def ref_clean_document(doc, open_radius=0, close_radius=0, smooth_shape="disk", min_component_area=0, keep_largest=False, fill_holes=0,
                       component_connectivity=8, area_rule="pixels", decode=C.decode_segmentation):
    """s2d_amd.clean_annotations.clean_document with the smoothing options on the host -> (doc, stats): the existing reference run on
    a document whose masks are smoothed, with `changed` widened to opened + closed > 0.  With both radii 0 it IS the existing one."""
    if ref_radius(open_radius, 100, 100) == 0 and ref_radius(close_radius, 100, 100) == 0:
        return C.ref_clean_document(doc, min_component_area, keep_largest, fill_holes, component_connectivity, area_rule, decode)
    stats = {"planes": 0, "planes_changed": 0, "pixels_removed": 0, "pixels_filled": 0, "annotations_dropped": 0, "frames_emptied": 0,
             "pixels_opened": 0, "pixels_closed": 0}
    video = "videos" in doc
    sizes = {r["id"]: (int(r["height"]), int(r["width"])) for r in doc["videos" if video else "images"]}

    def clean(seg, H, W):
        o, r, f, op, cl = ref_smooth_clean(decode(seg, H, W), ref_radius(open_radius, H, W), ref_radius(close_radius, H, W), smooth_shape,
                                           min_component_area, keep_largest, fill_holes, component_connectivity)
        stats["planes"] += 1
        stats["pixels_removed"] += r
        stats["pixels_filled"] += f
        stats["pixels_opened"] += op
        stats["pixels_closed"] += cl
        stats["planes_changed"] += int(r + f + op + cl > 0)
        return o, r + f + op + cl > 0

    anns = []
    for ann in doc["annotations"]:
        if ann.get("iscrowd", 0) == 1:
            anns.append(ann)
            continue
        if video:
            H, W = sizes[ann["video_id"]]
            new = None
            for t, seg in enumerate(ann["segmentations"]):
                if seg is None:
                    continue
                o, changed = clean(seg, H, W)
                if not changed:
                    continue
                if new is None:
                    new = dict(ann, segmentations=list(ann["segmentations"]), bboxes=list(ann["bboxes"]), areas=list(ann["areas"]))
                if o.any():
                    new["segmentations"][t], new["bboxes"][t], new["areas"][t] = \
                        C.encode_mask(o), [float(v) for v in C.tight_box(o)], int(o.sum())
                else:
                    new["segmentations"][t] = new["bboxes"][t] = new["areas"][t] = None
                    stats["frames_emptied"] += 1
            if new is None:
                anns.append(ann)
            elif all(s is None for s in new["segmentations"]):
                stats["annotations_dropped"] += 1
            else:
                anns.append(new)
        else:
            H, W = sizes[ann["image_id"]]
            o, changed = clean(ann["segmentation"], H, W)
            if not changed:
                anns.append(ann)
            elif not o.any():
                stats["annotations_dropped"] += 1
            else:
                box = [float(v) for v in C.tight_box(o)]
                anns.append(dict(ann, segmentation=C.encode_mask(o), bbox=box, area=box[2] * box[3] if area_rule == "bbox" else int(o.sum())))
    out = {k: v for k, v in doc.items() if k != "annotations"}
    out["annotations"] = anns
    return out, stats


def ref_device_fn(decode=C.decode_segmentation):
    """a device_fn for clean_document made of the references, for either form of opts"""
    from types import SimpleNamespace

    def fn(chunk, opts):
        if len(opts) == 4:
            return C.ref_device_fn(decode)(chunk, opts)
        min_area, largest, conn, hole, open_spec, close_spec, shape = opts
        cols = {k: [] for k in ("removed", "filled", "opened", "closed")}
        sel, rles, areas, boxes = [], [], [], []
        for p, (segs, (H, W)) in enumerate(zip(chunk.segs, chunk.sizes)):
            o, r, f, op, cl = ref_smooth_clean(decode(segs[0], H, W), ref_radius(open_spec, H, W), ref_radius(close_spec, H, W), shape,
                                               min_area, largest, hole, conn)
            for k, v in zip(cols, (r, f, op, cl)):
                cols[k].append(v)
            if r + f + op + cl > 0:
                sel.append(p), rles.append(C.encode_mask(o)), areas.append(int(o.sum())), boxes.append(C.tight_box(o))
        return SimpleNamespace(sel=np.array(sel, np.int64), rles=rles, areas=np.array(areas, np.int64),
                               boxes=np.array(boxes, np.float64).reshape(-1, 4), **{k: np.array(v) for k, v in cols.items()})
    return fn


# ---------------------------------------------------------------------------------------------------------------- constructed cases
def whisker(H=24, W=70):
    """a 10 x 12 object with a 40-pixel-long, 1-pixel-wide whisker attached: ONE component, so no min_area removes the whisker"""
    m = np.zeros((H, W), bool)
    m[6:16, 4:16] = True
    m[10, 16:56] = True
    return m


def whisker_object(H=24, W=70):
    m = np.zeros((H, W), bool)
    m[6:16, 4:16] = True
    return m


def crack(H=24, W=40):
    """a 12 x 22 object split into two components by a 2-pixel crack: neither side is a hole"""
    m = np.zeros((H, W), bool)
    m[5:17, 6:28] = True
    m[:, 16:18] = False
    return m


def edge_rect(H, W, edge, h=6, w=10):
    """an h x w (along the edge) rectangle that touches the named image edge, away from the corners"""
    m = np.zeros((H, W), bool)
    if edge == "top":
        m[:h, 5:5 + w] = True
    elif edge == "bottom":
        m[H - h:, 5:5 + w] = True
    elif edge == "left":
        m[5:5 + w, :h] = True
    else:
        m[5:5 + w, W - h:] = True
    return m


def edge_strip(H, W, edge):
    """a 1-pixel strip along the named image edge, corner to corner"""
    m = np.zeros((H, W), bool)
    if edge == "top":
        m[0] = True
    elif edge == "bottom":
        m[H - 1] = True
    elif edge == "left":
        m[:, 0] = True
    else:
        m[:, W - 1] = True
    return m


EDGES = ("top", "bottom", "left", "right")


def blobs(H, W, rng, n=None):
    """seeded points dilated by a disk of 3"""
    m = np.zeros((H, W), bool)
    n = max(1, H * W // 150) if n is None else n
    m[rng.integers(0, H, n), rng.integers(0, W, n)] = True
    return dilate(m, 3)


def size_list(rows):
    """the sizes of the GPU file's first group; rows = morph_tile(r)[0]: (rows + 1) x 40 crosses a row tile, 3 x 1030 a word tile"""
    return [(1, 1), (1, 40), (40, 1), (5, 7), (31, 33), (33, 31), (64, 64), (37, 97), (3, 1030), (rows + 1, 40)]


def size_chunk(rows, seed=0):
    """-> list of bool planes: for every size a random plane at density 0.1 and 0.9 and a plane of blobs"""
    rng = np.random.default_rng(seed)
    planes = []
    for H, W in size_list(rows):
        planes += [rng.random((H, W)) < 0.1, rng.random((H, W)) < 0.9, blobs(H, W, rng)]
    return planes


# ---------------------------------------------------------------------------------------------------------------- documents
def ragged_mask(H, W, rng):
    """an ellipse with a whisker to the right, a 2-pixel crack through it, pinholes and speckle"""
    m = C.speckled_mask(H, W, rng, speckle=0.004, pinholes=0.01)
    ys, xs = np.nonzero(m)
    cy, cx = int(np.median(ys)), int(np.median(xs))
    m[cy, cx:min(W, cx + W // 2)] = True
    m[:, max(cx - 3, 0):max(cx - 1, 1)] = False
    return m


def make_coco_doc(seed=0):
    """plane_components_refs.make_coco_doc with ragged masks added: one per image, and one solid rectangle at the image edge that only
    the default-border rule leaves whole -> (doc, masks by annotation id)"""
    doc, masks = C.make_coco_doc(seed)
    rng = np.random.default_rng(seed + 100)
    anns = list(doc["annotations"])
    for img in doc["images"]:
        H, W = img["height"], img["width"]
        solid = np.zeros((H, W), bool)
        solid[:max(H // 2, 1), :max(W // 2, 1)] = True
        for m in (ragged_mask(H, W, rng), solid):
            aid = 100 + len(anns)
            anns.append({"id": aid, "image_id": img["id"], "category_id": 1, "iscrowd": 0, "segmentation": C.encode_mask(m),
                         "bbox": [float(v) for v in C.tight_box(m)], "area": int(m.sum()), "score": 0.25})
            masks[aid] = m
    return dict(doc, annotations=anns), masks


def make_ytvis_doc(seed=0):
    """plane_components_refs.make_ytvis_doc with a track of ragged masks per video -> (doc, masks by (annotation id, frame))"""
    doc, masks = C.make_ytvis_doc(seed)
    rng = np.random.default_rng(seed + 100)
    anns = list(doc["annotations"])
    for v in doc["videos"]:
        H, W, T = v["height"], v["width"], v["length"]
        aid = 50 + len(anns)
        ms = [ragged_mask(H, W, rng) for _ in range(T)]
        for t, m in enumerate(ms):
            masks[(aid, t)] = m
        anns.append({"id": aid, "video_id": v["id"], "category_id": 1, "iscrowd": 0, "height": H, "width": W, "length": T,
                     "segmentations": [C.encode_mask(m) for m in ms], "bboxes": [[float(x) for x in C.tight_box(m)] for m in ms],
                     "areas": [int(m.sum()) for m in ms]})
    return dict(doc, annotations=anns), masks
