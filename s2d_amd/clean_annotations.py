"""Mask cleanup for annotation files: every mask of a COCO image document or a YTVIS document goes through the connected-component
cleanup of s2d_amd/plane_components.py on the device, and the masks it changed are written back as compressed RLE.

    python -m s2d_amd.clean_annotations --ann in.json --save-path out.json [--min-component-area N] [--keep-largest]
        [--fill-holes N|all] [--component-connectivity 4|8] [--open R] [--close R] [--smooth-shape disk|square]
        [--area-rule pixels|bbox]

The masks of a results.json come from thresholded logits: they carry speckle and pinholes, whiskers and cracks, every self-training
round feeds them back, and the tight boxes the merges write grow with every stray blob.  The rule is fill(filter(close(open(mask)))).
Smoothing first (plane_morph.py states it): --open R removes what a disk (or square) of radius R does not fit into -- a 1-pixel
whisker on an object, which no component rule sees --, then --close R closes the cracks and bays it does not fit into; R is N pixels
or X% of the image diagonal (the rule of the Boundary IoU band), at most 64 pixels, and the border rule keeps a mask at the image edge
whole.  Then plane_components.py's fill(filter(.)) on the smoothed mask: components under --min-component-area pixels go (with
--keep-largest all but the largest), then holes of at most --fill-holes pixels are set, so what is written still has no component
under the one and no hole up to the other; the connectivity option does not touch the smoothing.  The rule is THIS PROJECT'S OWN: the
reference cleans nothing, so with every option off (the default) nothing is launched and the document is returned as it came.  The
same options are on `python -m s2d_amd.selftrain`, `s2d_amd.selftrain_video` and
`s2d_amd.keymask.results_to_annotations` (add_cleanup_arguments / cleanup_options), where the cleanup is a post-pass over the
merged document just before it is written: the merge and keep rules see the masks as they came.

What is written:
  * the kind of document is found the way `train --train-format auto` finds it (data.image_clip.detect_train_format);
  * an unchanged mask keeps its `segmentation` object, `bbox` and `area` untouched, and an annotation none of whose masks changed is
    the SAME object in the output; the input document is not modified;
  * a changed mask becomes compressed RLE (also when it was a polygon or uncompressed RLE).  In a COCO image document `bbox` becomes
    the tight box (floats) and `area` the pixel count, or bbox w * h under area_rule="bbox" (what selftrain.py writes, the reference's
    quirk); in a YTVIS document `bboxes[t]` and `areas[t]` are set;
  * a frame that becomes empty becomes None in `segmentations`, `bboxes` and `areas`; an annotation with no set pixel left is dropped;
    ids are never renumbered; `iscrowd = 1` annotations are left alone.

Device side, per chunk of masks of different sizes: stage (rle_ragged.stage_rle_ragged), decode (decode_ragged), with smoothing on
ops.morph_planes at the per-plane radii and the per-plane difference to the decoded plane (plane_morph.plane_diff_counts), clean in
place (ops.clean_planes), one read-back of the per-plane counts, then encode_ragged over the planes with a non-zero count only,
whose count pass also gives their areas and tight boxes.  Device memory is bounded by CLEAN_CHUNK_WORDS plus the largest
single plane, never by the file: a plane over the bound is a chunk of its own."""
import argparse
import json
import time
from types import SimpleNamespace

import numpy as np

CLEAN_CHUNK_WORDS = 5 << 19      # 2.6 M words = 84 M pixels: 12 bytes per pixel of labels and workspace stay under 1 GiB
FILL_ALL = 2 ** 31 - 1
AREA_RULES = ("pixels", "bbox")
STAT_KEYS = ("planes", "planes_changed", "pixels_removed", "pixels_filled", "annotations_dropped", "frames_emptied")
SMOOTH_STAT_KEYS = ("pixels_opened", "pixels_closed")      # beside STAT_KEYS when --open / --close is on: original vs smoothed mask


# ---------------------------------------------------------------------------------------------------------------- options
def _fill_holes(text):
    if str(text).lower() == "all":
        return FILL_ALL
    v = int(text)
    if v < 0:
        raise argparse.ArgumentTypeError(f"--fill-holes {text}: a pixel count >= 0, or `all`")
    return v


def _radius(text):
    from .plane_morph import parse_radius
    try:
        r = parse_radius(text)
    except ValueError as e:
        raise argparse.ArgumentTypeError(str(e))
    return r if isinstance(r, int) else str(text).strip()


def add_cleanup_arguments(ap):
    """the cleanup options, the same on every command line that writes an annotation file"""
    g = ap.add_argument_group("mask cleanup (this project's own; off by default: the reference cleans nothing)")
    g.add_argument("--min-component-area", type=int, default=0, help="remove connected components of fewer pixels (0: off)")
    g.add_argument("--keep-largest", action="store_true", help="keep only the largest component of every mask")
    g.add_argument("--fill-holes", type=_fill_holes, default=0, metavar="N|all", help="fill holes of at most N pixels (0: off)")
    g.add_argument("--component-connectivity", type=int, choices=(4, 8), default=8,
                   help="connectivity of the set pixels; holes use the complementary one")
    g.add_argument("--open", type=_radius, default=0, metavar="R", dest="open_radius",
                   help="morphological opening at radius R before the component rules: N pixels or X%% of the image diagonal (0: off)")
    g.add_argument("--close", type=_radius, default=0, metavar="R", dest="close_radius",
                   help="morphological closing at radius R after the opening: N pixels or X%% of the image diagonal (0: off)")
    g.add_argument("--smooth-shape", choices=("disk", "square"), default="disk", help="structuring element of --open / --close")
    return ap


def cleanup_options(args):
    """parsed arguments -> the keyword arguments of clean_document, checked"""
    opts = {"min_component_area": args.min_component_area, "keep_largest": bool(args.keep_largest), "fill_holes": args.fill_holes,
            "component_connectivity": args.component_connectivity}
    smooth = _smooth_options(getattr(args, "open_radius", 0), getattr(args, "close_radius", 0), getattr(args, "smooth_shape", "disk"))
    if smooth:                                                           # with both radii 0 the dict is the four keys it always was
        opts.update(open_radius=smooth[0], close_radius=smooth[1], smooth_shape=smooth[2])
    _options(**opts)
    return opts


def _smooth_options(open_radius=0, close_radius=0, smooth_shape="disk"):
    """-> () when both radii are 0, else (open_radius, close_radius, smooth_shape), checked: a radius is N or "X%" (plane_morph)"""
    from .plane_morph import SHAPES, parse_radius
    if smooth_shape not in SHAPES:
        raise ValueError(f"smooth_shape {smooth_shape!r}: one of {SHAPES}")
    if not (parse_radius(open_radius) > 0 or parse_radius(close_radius) > 0):
        return ()
    return open_radius, close_radius, smooth_shape


def _options(min_component_area=0, keep_largest=False, fill_holes=0, component_connectivity=8, open_radius=0, close_radius=0,
             smooth_shape="disk"):
    """-> (min_area, keep_largest, connectivity, max_hole_area), and with a non-zero radius + (open_radius, close_radius, smooth_shape)"""
    from .plane_components import component_hole_options
    return component_hole_options({"min_component_area": min_component_area, "keep_largest": keep_largest,
                                   "component_connectivity": component_connectivity, "max_hole_area": fill_holes}) \
        + _smooth_options(open_radius, close_radius, smooth_shape)


def cleanup_is_on(opts):
    """does a cleanup_options dict (or None) ask for anything"""
    if not opts:
        return False
    return _is_on(_options(**opts))


def _is_on(opts):
    return opts[0] > 0 or opts[1] or opts[3] > 0 or len(opts) > 4


# ---------------------------------------------------------------------------------------------------------------- device side
def device_clean(chunk, opts, device=None, seconds=None):
    """the device side of one chunk (SimpleNamespace: segs = one list of ONE segmentation per plane, sizes, names) with opts =
    (min_area, keep_largest, connectivity, max_hole_area) -> SimpleNamespace(removed int [P], filled int [P], sel: the changed planes,
    rles / areas / boxes: their new RLE dicts, pixel counts and tight boxes).  With smoothing on opts is that + (open_radius,
    close_radius, smooth_shape): the radii become pixels per plane from chunk.sizes (a radius over 64 raises, naming the image, before
    anything is launched), the planes are opened and closed before the clean, and the result gains opened int [P] / closed int [P]:
    the pixels of the decoded plane the smoothing cleared / set; removed and filled count against the smoothed plane.  seconds: a
    dict that collects device-inclusive times."""
    import torch
    from . import coco_eval, ops
    from .rle_ragged import decode_ragged, encode_ragged, stage_rle_ragged
    dev = coco_eval._device(device)

    def tick(name, t0):
        if seconds is not None:
            torch.cuda.synchronize(dev)
            seconds[name] = seconds.get(name, 0.0) + time.perf_counter() - t0
        return time.perf_counter()

    min_area, largest, conn, hole = opts[:4]
    radii = []
    if len(opts) > 4:
        from .plane_morph import smooth_radius
        radii = [np.array([smooth_radius(spec, H, W, name) for (H, W), name in zip(chunk.sizes, chunk.names)], np.int32) for spec in opts[4:6]]
    t0 = time.perf_counter()
    staged = stage_rle_ragged(chunk.segs, chunk.sizes, names=chunk.names)
    t0 = tick("stage", t0)
    dec = decode_ragged(staged, dev)
    t0 = tick("decode", t0)
    bits, smoothed = dec.bits, []
    if radii:
        from .plane_morph import plane_diff_counts
        for op, rad in zip(("open", "close"), radii):
            if rad.any():
                bits = ops.morph_planes(bits, staged.plane, op, rad, opts[6])[0]
        smoothed = list(plane_diff_counts(dec.bits, bits, staged.plane))
        t0 = tick("smooth", t0)
    out, removed, filled = ops.clean_planes(bits, staged.plane, min_area, largest, hole, conn, out=bits)
    counts = torch.stack([removed, filled] + smoothed).cpu().numpy()     # the one read-back of the clean: which planes changed
    t0 = tick("clean", t0)
    sel = np.flatnonzero(counts.sum(0) > 0)
    rles, areas, boxes = encode_ragged(out, staged.plane, sel)
    tick("encode", t0)
    if seconds is not None:
        seconds["device_bytes"] = max(seconds.get("device_bytes", 0), int(torch.cuda.max_memory_allocated(dev)))
    r = SimpleNamespace(removed=counts[0], filled=counts[1], sel=sel, rles=rles, areas=areas, boxes=boxes)
    if radii:
        r.opened, r.closed = counts[2], counts[3]
    return r


# ---------------------------------------------------------------------------------------------------------------- the document
def _planes(doc, video):
    """-> the masks to clean, in file order: (annotation index, frame or None, segmentation, H, W, name)"""
    key = "video_id" if video else "image_id"
    sizes = {r["id"]: (int(r["height"]), int(r["width"])) for r in doc["videos" if video else "images"]}
    units = []
    for k, ann in enumerate(doc["annotations"]):
        if ann.get("iscrowd", 0) == 1:
            continue
        if ann.get(key) not in sizes:
            raise ValueError(f"annotation {ann.get('id')}: {key} {ann.get(key)!r} is not in the document")
        H, W = sizes[ann[key]]
        if video:
            for t, seg in enumerate(ann["segmentations"]):
                if seg is not None:
                    units.append((k, t, seg, H, W, f"{ann[key]} (annotation {ann.get('id')}, frame {t})"))
        else:
            if not ann.get("segmentation"):
                raise ValueError(f"annotation {ann.get('id')} of image {ann[key]}: no segmentation")
            units.append((k, None, ann["segmentation"], H, W, f"{ann[key]} (annotation {ann.get('id')})"))
    return units


def _chunks(units):
    """the masks cut at CLEAN_CHUNK_WORDS; a mask over the bound is a chunk of its own"""
    chunk, words = [], 0
    for u in units:
        w = (u[3] * u[4] + 31) // 32
        if chunk and words + w > CLEAN_CHUNK_WORDS:
            yield chunk
            chunk, words = [], 0
        chunk.append(u)
        words += w
    if chunk:
        yield chunk


def clean_document(doc, min_component_area=0, keep_largest=False, fill_holes=0, component_connectivity=8, area_rule="pixels",
                   device=None, device_fn=None, seconds=None, open_radius=0, close_radius=0, smooth_shape="disk"):
    """a loaded COCO image or YTVIS annotation document -> (the cleaned document, stats) (module docstring).  device_fn: (chunk, opts)
    -> what device_clean returns replaces the device side, so the host logic runs without a device; seconds: a dict that collects the
    phase times (stage, decode, smooth, clean, encode: device-inclusive; assemble).  stats: the counts named by STAT_KEYS, and with
    open_radius / close_radius (N, or "X%" of the image diagonal) non-zero those of SMOOTH_STAT_KEYS."""
    from .data.image_clip import detect_train_format
    opts = _options(min_component_area, keep_largest, fill_holes, component_connectivity, open_radius, close_radius, smooth_shape)
    smooth = len(opts) > 4
    if area_rule not in AREA_RULES:
        raise ValueError(f"area_rule must be one of {AREA_RULES}, not {area_rule!r}")
    stats = dict.fromkeys(STAT_KEYS, 0)
    if not _is_on(opts):
        return doc, stats
    if smooth:
        stats.update(dict.fromkeys(SMOOTH_STAT_KEYS, 0))
    if device_fn is None:
        device_fn = lambda chunk, o: device_clean(chunk, o, device, seconds)      # noqa: E731
    t0 = time.perf_counter()
    video = detect_train_format(doc) != "coco_image"
    units = _planes(doc, video)
    new = {}                                                             # annotation index -> its changed copy
    host = time.perf_counter() - t0
    for part in _chunks(units):
        chunk = SimpleNamespace(units=part, segs=[[u[2]] for u in part], sizes=[(u[3], u[4]) for u in part], names=[u[5] for u in part])
        r = device_fn(chunk, opts)
        t0 = time.perf_counter()
        removed, filled, sel = np.asarray(r.removed).reshape(-1), np.asarray(r.filled).reshape(-1), np.asarray(r.sel).reshape(-1)
        changed = removed + filled
        if smooth:
            opened, closed = np.asarray(r.opened).reshape(-1), np.asarray(r.closed).reshape(-1)
            if len(opened) != len(part) or len(closed) != len(part):
                raise ValueError(f"device_fn returned {len(opened)} / {len(closed)} smoothing counts for {len(part)} planes")
            changed = changed + opened + closed
            stats["pixels_opened"] += int(opened.sum())
            stats["pixels_closed"] += int(closed.sum())
        if len(removed) != len(part) or len(filled) != len(part) or not np.array_equal(sel, np.flatnonzero(changed > 0)) \
                or not len(r.rles) == len(r.areas) == len(r.boxes) == len(sel):
            raise ValueError(f"device_fn returned {len(removed)} / {len(filled)} counts and {len(sel)} changed planes for {len(part)} planes")
        stats["planes"] += len(part)
        stats["planes_changed"] += len(sel)
        stats["pixels_removed"] += int(removed.sum())
        stats["pixels_filled"] += int(filled.sum())
        for j, p in enumerate(sel):
            k, t = part[p][0], part[p][1]
            area, box = int(r.areas[j]), [float(v) for v in r.boxes[j]]
            a = new.get(k)
            if a is None:
                a = new[k] = dict(doc["annotations"][k])
                if video:
                    n = len(a["segmentations"])
                    a["segmentations"] = list(a["segmentations"])
                    a["bboxes"], a["areas"] = list(a.get("bboxes") or [None] * n), list(a.get("areas") or [None] * n)
            if video:
                if area:
                    a["segmentations"][t], a["bboxes"][t], a["areas"][t] = r.rles[j], box, area
                else:
                    a["segmentations"][t] = a["bboxes"][t] = a["areas"][t] = None
                    stats["frames_emptied"] += 1
            elif area:
                a["segmentation"], a["bbox"] = r.rles[j], box
                a["area"] = box[2] * box[3] if area_rule == "bbox" else area
            else:
                new[k] = None
        host += time.perf_counter() - t0
    t0 = time.perf_counter()
    anns = []
    for k, ann in enumerate(doc["annotations"]):
        if k not in new:
            anns.append(ann)
            continue
        a = new[k]
        if a is None or (video and all(s is None for s in a["segmentations"])):
            stats["annotations_dropped"] += 1
        else:
            anns.append(a)
    out = dict(doc)
    out["annotations"] = anns
    if seconds is not None:
        seconds["assemble"] = seconds.get("assemble", 0.0) + host + time.perf_counter() - t0
    return out, stats


def clean_merged(doc, cleanup, area_rule="pixels", device=None):
    """the post-pass of the drivers that write an annotation file: clean_document when `cleanup` (a cleanup_options dict, or None)
    asks for anything, with the stats printed; otherwise the document itself, with nothing launched"""
    if not cleanup_is_on(cleanup):
        return doc
    doc, stats = clean_document(doc, area_rule=area_rule, device=device, **cleanup)
    print("Cleanup: " + "; ".join(f"{stats[k]} {k.replace('_', ' ')}" for k in stats) + ".")
    return doc


def clean_file(ann, save_path, area_rule="pixels", device=None, device_fn=None, seconds=None, **options):
    """the command line on paths -> (the written document, stats)"""
    t0 = time.perf_counter()
    with open(ann) as fh:
        doc = json.load(fh)
    t_json = time.perf_counter() - t0
    doc, stats = clean_document(doc, area_rule=area_rule, device=device, device_fn=device_fn, seconds=seconds, **options)
    t0 = time.perf_counter()
    with open(save_path, "w") as fh:
        json.dump(doc, fh)
    if seconds is not None:
        seconds["json"] = seconds.get("json", 0.0) + t_json + time.perf_counter() - t0
    return doc, stats


def build_parser():
    ap = argparse.ArgumentParser(description="Clean the masks of a COCO image or YTVIS annotation file (opening / closing, connected components, holes).")
    ap.add_argument("--ann", required=True, help="the annotation JSON to clean")
    ap.add_argument("--save-path", required=True, help="where the cleaned annotation JSON is written")
    ap.add_argument("--area-rule", choices=AREA_RULES, default="pixels",
                    help="`area` of a changed COCO image annotation: its pixel count (default), or bbox w * h as selftrain writes it")
    return add_cleanup_arguments(ap)


def main(argv=None):
    a = build_parser().parse_args(argv)
    doc, stats = clean_file(a.ann, a.save_path, a.area_rule, **cleanup_options(a))
    print("Done: {} anns; ".format(len(doc["annotations"])) + "; ".join(f"{stats[k]} {k.replace('_', ' ')}" for k in stats) + ".")


if __name__ == "__main__":
    main()
