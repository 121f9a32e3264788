"""Host references of the ragged bit-plane component ops (s2d_amd/plane_components.py), of the ragged RLE encoder
(s2d_amd/rle_ragged.encode_ragged) and of the annotation cleanup built on them (s2d_amd/clean_annotations.py), with the constructed
cases of their tests.  None of them restates the kernel: labels are scipy.ndimage.label renamed to first-pixel labels, holes are
scipy.ndimage.binary_fill_holes with the size limit applied through a label of the holes, the RLE strings come from a numpy
column-major encoder with maskApi.c's rleToString written out, and `ref_clean_document` is built from those.

The rule (s2d_amd/plane_components.py): cleanup = fill(filter(plane)).  filter keeps a component of set pixels iff area >= min_area
and (keep_largest) it is the largest of its plane, equal areas to the lower first pixel.  fill sets the holes -- zero components
under the complementary connectivity that touch no border row or column -- of at most max_hole_area pixels."""
import numpy as np
from scipy import ndimage

FILL_ALL = 2 ** 31 - 1


def structure(conn):
    if conn not in (4, 8):
        raise ValueError(f"connectivity {conn}: 4 or 8")
    return ndimage.generate_binary_structure(2, 1 if conn == 4 else 2)


# ---------------------------------------------------------------------------------------------------------------- the flat layout
def pack_planes(masks, set_padding=False, gap_words=0):
    """masks: list of bool [H, W] -> (bits int32 [words], plane int64 [P, 4] = {word0, H, W, 0}): pixel i = y*W + x of a plane in word
    i // 32, bit i % 32, the planes back to back (gap_words unused words of all ones between them).  set_padding: the padding bits of
    every plane's last word are 1"""
    words, rows = [], []
    w0 = 0
    for m in masks:
        m = np.asarray(m, bool)
        H, W = m.shape
        n = (H * W + 31) // 32
        flat = np.zeros(32 * n, bool)
        flat[:H * W] = m.reshape(-1)
        if set_padding:
            flat[H * W:] = True
        words.append(np.packbits(flat, bitorder="little").view(np.uint32))
        rows.append((w0, H, W, 0))
        w0 += n
        if gap_words:
            words.append(np.full(gap_words, 0xffffffff, np.uint32))
            w0 += gap_words
    bits = np.concatenate(words) if words else np.zeros(0, np.uint32)
    return bits.view(np.int32).copy(), np.asarray(rows, np.int64).reshape(-1, 4)


def unpack_plane(bits, row, with_padding=False):
    """-> bool [H, W] of a table row; with_padding: (mask, the padding bits of the last word as a bool array)"""
    w0, H, W = int(row[0]), int(row[1]), int(row[2])
    n = (H * W + 31) // 32
    flat = np.unpackbits(np.asarray(bits)[w0:w0 + n].view(np.uint8), bitorder="little").astype(bool)
    m = flat[:H * W].reshape(H, W)
    return (m, flat[H * W:]) if with_padding else m


def expected_per_pixel(per_plane, plane, words):
    """per-plane [H, W] arrays -> the [32 * words] array with 0 at positions of no pixel"""
    out = np.zeros(32 * words, np.int32)
    for a, r in zip(per_plane, plane):
        w0, H, W = int(r[0]), int(r[1]), int(r[2])
        out[32 * w0:32 * w0 + H * W] = np.asarray(a).reshape(-1)
    return out


# ---------------------------------------------------------------------------------------------------------------- labels
def ref_labels(mask, value, conn):
    """bool [H, W] -> (labels int32 [H, W], area int32 [H, W]) of the pixels equal to `value`: 1 + the flat index of the component's
    first pixel, and the component's pixel count at that pixel"""
    m = np.asarray(mask, bool) == bool(value)
    H, W = m.shape
    lab, k = ndimage.label(m, structure(conn))
    flat = lab.reshape(-1)
    pos = np.flatnonzero(flat)
    first = np.full(k + 1, H * W, np.int64)
    np.minimum.at(first, flat[pos], pos)
    labels, area = np.zeros(H * W, np.int32), np.zeros(H * W, np.int32)
    labels[pos] = first[flat[pos]] + 1
    area[first[1:]] = np.bincount(flat, minlength=k + 1)[1:]
    return labels.reshape(H, W), area.reshape(H, W)


def flood_labels(mask, value, conn):
    """the same by a brute-force flood fill in raster order (tiny planes only): the check of ref_labels"""
    m = np.asarray(mask, bool) == bool(value)
    H, W = m.shape
    labels, area = np.zeros((H, W), np.int32), np.zeros((H, W), np.int32)
    nb = [(-1, 0), (1, 0), (0, -1), (0, 1)] + ([(-1, -1), (-1, 1), (1, -1), (1, 1)] if conn == 8 else [])
    for y0 in range(H):
        for x0 in range(W):
            if not m[y0, x0] or labels[y0, x0]:
                continue
            name, stack, n = y0 * W + x0 + 1, [(y0, x0)], 0
            labels[y0, x0] = name
            while stack:
                y, x = stack.pop()
                n += 1
                for dy, dx in nb:
                    yy, xx = y + dy, x + dx
                    if 0 <= yy < H and 0 <= xx < W and m[yy, xx] and not labels[yy, xx]:
                        labels[yy, xx] = name
                        stack.append((yy, xx))
            area[y0, x0] = n
    return labels, area


def ref_filter(mask, min_area, keep_largest, conn):
    m = np.asarray(mask, bool)
    if not (min_area > 0 or keep_largest):
        return m.copy()
    labels, area = ref_labels(m, 1, conn)
    roots = np.flatnonzero(area.reshape(-1))                              # ascending first pixels
    a = area.reshape(-1)[roots]
    keep = a >= min_area
    if keep_largest and len(roots):
        best = np.lexsort((roots, -a.astype(np.int64)))[0]                # largest area, then lowest first pixel
        only = np.zeros(len(roots), bool)
        only[best] = True
        keep &= only
    return m & np.isin(labels, roots[keep] + 1)


def ref_fill(mask, max_hole_area, conn):
    """conn: the connectivity of the SET pixels; the holes are labelled under the complementary one"""
    m = np.asarray(mask, bool)
    if max_hole_area <= 0:
        return m.copy()
    filled = ndimage.binary_fill_holes(m, structure(4 if conn == 8 else 8))     # cross for foreground 8, 3 x 3 ones for foreground 4
    holes = filled & ~m
    lab, k = ndimage.label(holes, structure(4 if conn == 8 else 8))
    size = np.bincount(lab.reshape(-1), minlength=k + 1)
    ok = size <= max_hole_area
    ok[0] = False
    return m | ok[lab]


def ref_clean(mask, min_area=0, keep_largest=False, max_hole_area=0, conn=8):
    """-> (out bool [H, W], removed, filled)"""
    m = np.asarray(mask, bool)
    f = ref_filter(m, min_area, keep_largest, conn)
    o = ref_fill(f, max_hole_area, conn)
    return o, int((m & ~f).sum()), int((o & ~f).sum())


def flood_holes(mask, conn):
    """the zero components (complementary connectivity) with no pixel on the border, by flood fill: -> bool [H, W]"""
    m = np.asarray(mask, bool)
    H, W = m.shape
    labels, _ = flood_labels(m, 0, 4 if conn == 8 else 8)
    edge = np.zeros((H, W), bool)
    edge[0], edge[-1], edge[:, 0], edge[:, -1] = True, True, True, True
    open_names = np.unique(labels[edge & ~m])
    return ~m & ~np.isin(labels, open_names)


# ---------------------------------------------------------------------------------------------------------------- RLE in numpy
def rle_counts(mask):
    """bool [H, W] -> run lengths of the column-major flattened mask, alternating 0s / 1s, starting with the zero run"""
    flat = np.asarray(mask, bool).reshape(-1, order="F")
    change = np.flatnonzero(flat[1:] != flat[:-1]) + 1
    edges = np.concatenate([[0], change, [flat.size]])
    counts = np.diff(edges)
    if flat.size and flat[0]:
        counts = np.concatenate([[0], counts])
    return counts.astype(np.int64)


def rle_to_string(counts):
    """maskApi.c rleToString: counts[i > 2] as a difference to counts[i - 2]; 5 bits per char, bit 5 = more, + 48"""
    out = bytearray()
    for i, c in enumerate(counts):
        x = int(c)
        if i > 2:
            x -= int(counts[i - 2])
        more = True
        while more:
            ch = x & 0x1f
            x >>= 5
            more = (x != -1) if (ch & 0x10) else (x != 0)
            if more:
                ch |= 0x20
            out.append(ch + 48)
    return bytes(out)


def rle_from_string(s):
    """maskApi.c rleFrString -> counts"""
    s = s.encode() if isinstance(s, str) else bytes(s)
    counts, p = [], 0
    while p < len(s):
        x, k, more = 0, 0, True
        while more:
            c = s[p] - 48
            x |= (c & 0x1f) << (5 * k)
            more = bool(c & 0x20)
            p += 1
            k += 1
            if not more and (c & 0x10):
                x |= -1 << (5 * k)
        if len(counts) > 2:
            x += counts[-2]
        counts.append(x)
    return np.asarray(counts, np.int64)


def rle_decode(counts, H, W):
    flat = np.zeros(H * W, bool)
    ends = np.cumsum(counts)
    for i in range(1, len(counts), 2):
        flat[ends[i - 1]:ends[i]] = True
    return flat.reshape(W, H).T.copy()


def encode_mask(mask):
    """bool [H, W] -> {"size": [H, W], "counts": str}"""
    H, W = np.asarray(mask).shape
    return {"size": [int(H), int(W)], "counts": rle_to_string(rle_counts(mask)).decode("ascii")}


def decode_segmentation(seg, H, W):
    """an RLE dict (compressed or uncompressed) -> bool [H, W]; polygons are not decoded here"""
    c = seg["counts"]
    return rle_decode(np.asarray(c, np.int64) if isinstance(c, (list, tuple)) else rle_from_string(c), H, W)


def tight_box(mask):
    """-> [x, y, w, h] of the set pixels, [0, 0, 0, 0] for an empty mask (mask_util.toBbox)"""
    ys, xs = np.nonzero(mask)
    if len(ys) == 0:
        return [0, 0, 0, 0]
    return [int(xs.min()), int(ys.min()), int(xs.max() - xs.min() + 1), int(ys.max() - ys.min() + 1)]


# ---------------------------------------------------------------------------------------------------------------- the document
def ref_clean_document(doc, min_component_area=0, keep_largest=False, fill_holes=0, component_connectivity=8, area_rule="pixels",
                       decode=decode_segmentation):
    """s2d_amd.clean_annotations.clean_document on the host -> (doc, stats).  RLE segmentations only (decode may add polygons)."""
    stats = {"planes": 0, "planes_changed": 0, "pixels_removed": 0, "pixels_filled": 0, "annotations_dropped": 0, "frames_emptied": 0}
    if not (min_component_area > 0 or keep_largest or fill_holes > 0):
        return doc, stats
    video = "videos" in doc
    out = {k: v for k, v in doc.items() if k != "annotations"}
    anns = []

    def clean(seg, H, W):
        m = decode(seg, H, W)
        o, r, f = ref_clean(m, min_component_area, keep_largest, fill_holes, component_connectivity)
        stats["planes"] += 1
        stats["pixels_removed"] += r
        stats["pixels_filled"] += f
        stats["planes_changed"] += int(r + f > 0)
        return o, r + f > 0

    def area_of(o):
        box = [float(v) for v in tight_box(o)]
        return box, (box[2] * box[3] if area_rule == "bbox" else int(o.sum()))

    sizes = {r["id"]: (int(r["height"]), int(r["width"])) for r in doc["videos" if video else "images"]}
    for ann in doc["annotations"]:
        if ann.get("iscrowd", 0) == 1:
            anns.append(ann)
            continue
        if video:
            H, W = sizes[ann["video_id"]]
            new, any_change = None, False
            for t, seg in enumerate(ann["segmentations"]):
                if seg is None:
                    continue
                o, changed = clean(seg, H, W)
                if not changed:
                    continue
                if new is None:
                    new = dict(ann, segmentations=list(ann["segmentations"]), bboxes=list(ann["bboxes"]), areas=list(ann["areas"]))
                any_change = True
                if o.any():
                    box = tight_box(o)
                    new["segmentations"][t], new["bboxes"][t], new["areas"][t] = encode_mask(o), [float(v) for v in box], int(o.sum())
                else:
                    new["segmentations"][t] = new["bboxes"][t] = new["areas"][t] = None
                    stats["frames_emptied"] += 1
            if not any_change:
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
                box, area = area_of(o)
                anns.append(dict(ann, segmentation=encode_mask(o), bbox=box, area=area))
    out["annotations"] = anns
    return out, stats


# ---------------------------------------------------------------------------------------------------------------- constructed cases
def size_cases(th, tw):
    """the sizes of the issue's first group: every W of the list with a few H, every H with a few W -- (H, W) pairs, duplicates
    removed, all of which go into ONE chunk"""
    Ws = [1, 2, 31, 32, 33, 63, 64, 65, tw - 1, tw, tw + 1, 2 * tw + 5]
    Hs = [1, 2, th - 1, th, th + 1, 2 * th + 5]
    out = []
    for i, W in enumerate(Ws):
        for H in (Hs[i % len(Hs)], Hs[(i + 3) % len(Hs)], 2 * th + 5):
            out.append((H, W))
    for i, H in enumerate(Hs):
        for W in (Ws[i % len(Ws)], Ws[(i + 5) % len(Ws)], 2 * tw + 5):
            out.append((H, W))
    seen, uniq = set(), []
    for s in out:
        if s not in seen:
            seen.add(s)
            uniq.append(s)
    return uniq


def random_plane(H, W, rng, density=0.55):
    return rng.random((H, W)) < density


def size_chunk(th, tw, seed=0):
    """-> list of bool planes: a random plane of every size of size_cases, plus an empty, a full and a 1 x 1 plane"""
    rng = np.random.default_rng(seed)
    planes = [random_plane(H, W, rng, 0.45 + 0.2 * rng.random()) for H, W in size_cases(th, tw)]
    planes += [np.zeros((th + 3, tw + 3), bool), np.ones((th + 3, tw + 3), bool), np.ones((1, 1), bool), np.zeros((1, 1), bool)]
    return planes


def row_wrap(H, W):
    """column W-1 set on even rows, column 0 on odd rows: flat neighbours that are no neighbours in the plane (for W > 2)"""
    m = np.zeros((H, W), bool)
    m[0::2, W - 1] = True
    m[1::2, 0] = True
    return m


def spiral(H, W):
    """a one-pixel-wide spiral from (0, 0) to the centre, arms one empty pixel apart: ONE component under both connectivities"""
    m = np.zeros((H, W), bool)
    y = x = d = 0
    m[0, 0] = True
    steps = ((0, 1), (1, 0), (0, -1), (-1, 0))

    def free(yy, xx):
        return not (0 <= yy < H and 0 <= xx < W) or not m[yy, xx]

    def can(d):
        dy, dx = steps[d]
        return 0 <= y + dy < H and 0 <= x + dx < W and not m[y + dy, x + dx] and free(y + 2 * dy, x + 2 * dx)

    while True:
        if not can(d):
            d = (d + 1) % 4
            if not can(d):
                break
        y, x = y + steps[d][0], x + steps[d][1]
        m[y, x] = True
    return m


def comb(H, W):
    """a spine along the bottom row with a tooth on every other column up to row 0: one component whose teeth meet only in the
    last row of tiles"""
    m = np.zeros((H, W), bool)
    m[H - 1] = True
    m[:, 0::2] = True
    return m


def checkerboard(H, W):
    yy, xx = np.mgrid[0:H, 0:W]
    return (yy + xx) % 2 == 0


def corner_pair(th, tw, anti=False):
    """two pixels that touch only diagonally at the four-tile corner"""
    m = np.zeros((3 * th + 1, 3 * tw + 1), bool)
    if anti:
        m[th - 1, tw] = m[th, tw - 1] = True
    else:
        m[th - 1, tw - 1] = m[th, tw] = True
    return m


def merge_cases(th, tw):
    H, W = 3 * th + 1, 3 * tw + 1
    return {"spiral": spiral(H, W), "comb": comb(H, W), "checker": checkerboard(H, W), "corner": corner_pair(th, tw),
            "corner_anti": corner_pair(th, tw, True)}


def tie_plane(th, tw):
    """two components of 9 pixels (the first inside tile (0, 0), the second across a tile corner), one of 4 and one of 1"""
    m = np.zeros((3 * th + 1, 3 * tw + 1), bool)
    m[2:5, 2:5] = True
    m[th - 1:th + 2, tw - 1:tw + 2] = True
    m[2 * th + 3:2 * th + 5, 7:9] = True
    m[0, 3 * tw] = True
    return m


def ring(H, W, y0, x0, h, w, t=1):
    """a rectangle outline of thickness t with its top-left corner at (y0, x0)"""
    m = np.zeros((H, W), bool)
    m[y0:y0 + h, x0:x0 + w] = True
    m[y0 + t:y0 + h - t, x0 + t:x0 + w - t] = False
    return m


def hole_cases(th, tw):
    """name -> bool plane; the properties are proven in tests/test_plane_components_refs_cpu.py"""
    H, W = 2 * th + 5, 2 * tw + 5
    c = {}
    c["ring"] = ring(H, W, 3, 3, th + 4, tw + 4)                                        # a hole across tile borders
    nested = ring(H, W, 1, 1, H - 2, W - 2) | ring(H, W, 5, 5, H - 10, W - 10)          # a ring in a hole in a ring
    c["nested"] = nested
    op = ring(H, W, 0, 4, 9, 9)                                                         # its hole reaches row 0 through a gap
    op[0, 8] = False
    c["open"] = op
    dg = ring(H, W, 4, 4, 9, 9)                                                         # closed only diagonally: a corner pixel missing
    dg[4, 4] = False
    c["diagonal"] = dg
    isl = ring(H, W, 2, 2, th + 6, tw + 6, 2)                                           # an island of 2 pixels inside a ring
    isl[10, 10:12] = True
    c["island"] = isl
    return c


def blob_with_speckle(H, W, seed=0):
    """one large blob with pinholes, and speckle around it"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    m = ((yy - H / 2) / (H / 3)) ** 2 + ((xx - W / 2) / (W / 4)) ** 2 < 1
    m = m & ~(rng.random((H, W)) < 0.002)
    return m | (rng.random((H, W)) < 0.001)


# ---------------------------------------------------------------------------------------------------------------- documents
def speckled_mask(H, W, rng, speckle=0.01, pinholes=0.02):
    """an ellipse somewhere in the image with pinholes, and speckle around it"""
    yy, xx = np.mgrid[0:H, 0:W]
    cy, cx = rng.uniform(0.3, 0.7) * H, rng.uniform(0.3, 0.7) * W
    ry, rx = rng.uniform(0.15, 0.3) * H + 1, rng.uniform(0.15, 0.3) * W + 1
    m = ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 < 1
    return (m & ~(rng.random((H, W)) < pinholes)) | (rng.random((H, W)) < speckle)


def only_speckle(H, W, rng, p=0.01):
    """isolated single pixels (no two adjacent, diagonals included): any min_area > 1 empties the mask"""
    m = np.zeros((H, W), bool)
    m[1::3, 1::3] = rng.random(m[1::3, 1::3].shape) < 9 * p
    if not m.any():
        m[1, 1] = True
    return m


def uncompressed(mask):
    H, W = mask.shape
    return {"size": [int(H), int(W)], "counts": [int(c) for c in rle_counts(mask)]}


def make_coco_doc(seed=0, sizes=((37, 53), (64, 64), (90, 131), (33, 200), (120, 97), (5, 7))):
    """a COCO image document: per image a few speckled masks; one uncompressed RLE, one clean mask (unchanged by any option), one
    mask of speckle only (emptied by min_area > 1), one crowd annotation of speckle (left alone).  -> (doc, masks by annotation id)"""
    rng = np.random.default_rng(seed)
    images, anns, masks = [], [], {}
    for i, (H, W) in enumerate(sizes):
        images.append({"id": 10 + i, "height": H, "width": W, "file_name": f"{i}.jpg"})
        kinds = ["speckled"] * (1 + i % 3) + (["clean"] if i % 2 == 0 else []) + (["speckle"] if i == 2 else []) + (["crowd"] if i == 3 else [])
        for kind in kinds:
            if kind == "speckled":
                m = speckled_mask(H, W, rng)
            elif kind == "clean":
                m = np.zeros((H, W), bool)
                m[H // 4:H // 2 + 2, W // 4:W // 2 + 2] = True
            else:
                m = only_speckle(H, W, rng)
            aid = 100 + len(anns)
            box = tight_box(m)
            seg = uncompressed(m) if (len(anns) % 4 == 1) else encode_mask(m)
            anns.append({"id": aid, "image_id": 10 + i, "category_id": 1, "iscrowd": int(kind == "crowd"), "segmentation": seg,
                         "bbox": [float(v) for v in box], "area": int(m.sum()), "score": 0.5 + 0.01 * len(anns)})
            masks[aid] = m
    doc = {"info": {"description": "synthetic"}, "images": images, "categories": [{"id": 1, "name": "fg", "supercategory": "fg"}],
           "annotations": anns}
    return doc, masks


def make_ytvis_doc(seed=0, sizes=((40, 60, 4), (72, 128, 3), (31, 33, 5))):
    """a YTVIS document: per video two tracks with absent frames; one frame of speckle only (emptied by min_area > 1), one track
    of speckle only (dropped), one clean track.  -> (doc, masks by (annotation id, frame))"""
    rng = np.random.default_rng(seed)
    videos, anns, masks = [], [], {}
    for v, (H, W, T) in enumerate(sizes):
        videos.append({"id": 5 + v, "height": H, "width": W, "length": T, "file_names": [f"{v}/{t}.jpg" for t in range(T)]})
        for k, kind in enumerate(["speckled", "mixed", "speckle", "clean"][:2 + v]):
            aid = 50 + len(anns)
            segs, boxes, areas = [], [], []
            for t in range(T):
                if (t + k) % 4 == 3:
                    segs.append(None), boxes.append(None), areas.append(None)
                    continue
                if kind == "speckle" or (kind == "mixed" and t == 1):
                    m = only_speckle(H, W, rng)
                elif kind == "clean":
                    m = np.zeros((H, W), bool)
                    m[2:H // 2, 3:W // 2] = True
                else:
                    m = speckled_mask(H, W, rng)
                masks[(aid, t)] = m
                segs.append(encode_mask(m)), boxes.append([float(x) for x in tight_box(m)]), areas.append(int(m.sum()))
            anns.append({"id": aid, "video_id": 5 + v, "category_id": 1, "iscrowd": 0, "height": H, "width": W, "length": T,
                         "segmentations": segs, "bboxes": boxes, "areas": areas})
    doc = {"info": {}, "licenses": [], "videos": videos, "categories": [{"id": 1, "name": "fg"}], "annotations": anns}
    return doc, masks


def ref_device_fn(decode=decode_segmentation):
    """a device_fn for clean_document made of the references: (chunk, opts) -> what clean_annotations.device_clean returns"""
    from types import SimpleNamespace

    def fn(chunk, opts):
        min_area, largest, conn, hole = opts
        removed, filled, sel, rles, areas, boxes = [], [], [], [], [], []
        for p, (segs, (H, W)) in enumerate(zip(chunk.segs, chunk.sizes)):
            o, r, f = ref_clean(decode(segs[0], H, W), min_area, largest, hole, conn)
            removed.append(r), filled.append(f)
            if r + f > 0:
                sel.append(p), rles.append(encode_mask(o)), areas.append(int(o.sum())), boxes.append(tight_box(o))
        return SimpleNamespace(removed=np.array(removed), filled=np.array(filled), sel=np.array(sel, np.int64), rles=rles,
                               areas=np.array(areas, np.int64), boxes=np.array(boxes, np.float64).reshape(-1, 4))
    return fn
