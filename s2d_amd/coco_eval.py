"""COCO image evaluation (class-agnostic or per-category mask AP / box AP, AR): COCOeval restated without pycocotools, the
image-side sibling of ytvis_eval.py for models trained with `--train-format coco_image`.

pycocotools is on none of the project's machines, so COCOeval.computeIoU / evaluateImg / accumulate / summarize and maskApi.c's
bbIou are restated here as the maintainers know them: PARITY WITH PYCOCOTOOLS IS UNPINNED.  Polygon ground truth is rasterised by
the library's own centre-sample even-odd rule (data/image_clip.polygons_to_bits), not by frPoly's upsampled boundary walk, so such
masks can differ from pycocotools' at boundary pixels: published COCO numbers are comparable only up to that.

Per chunk of images (of different sizes) the work is three launches, however many images the chunk holds (csrc/coco_eval.hip):
the mask IoU of every (detection, ground truth) pair from bit planes -- exact integer intersections and areas, one float64 division,
`inter / area(det)` for a crowd ground truth --, or the box IoU in bbIou's operation order, and evaluateImg's greedy matching for
every (image[, category]) x area range x threshold.  RLE strings are parsed and decoded on the device (ytvis_eval.stage_rle /
decode_staged), polygons rasterised there.  `matcher="host"` runs the Python loop of YTVISEval._evaluate_video on the same
device-computed IoUs instead of the matching kernel: a reference for the tests and the throughput script, not a fallback.
Accumulation and the summary are YTVISEval's (COCOeval.accumulate / summarize).

Definitions.  ignore = iscrowd.  A ground truth's area is its annotation's `area` when present (as COCOeval uses it), else its
mask's pixel count (segm) or w*h of its box (bbox); its box is the annotation's `bbox` when present, else the tight box of its mask
(rleToBbox).  A detection's area is its mask's pixel count (segm) or w*h of its box (bbox); its box is the result's own `bbox` when
given, else the tight box of its mask.  Area ranges: all [0, 1e10], small [0, 32^2], medium [32^2, 96^2], large [96^2, 1e10].
Detection ids are result positions + 1 (loadRes).  Refused: results for an image the ground truth does not have; an RLE whose size
is not the image's; a "segm" result or annotation without a segmentation; a "bbox" one with neither `bbox` nor segmentation.

Boundary AP (opt-in: iou_type="boundary") scores contour quality, which mask IoU is nearly blind to on large objects: Cheng et
al., "Boundary IoU" (CVPR 2021) and the published mask_to_boundary routine, restated as in ytvis_eval.py.  A mask's band is
Bd = M & ~E, E = M eroded d times by a 3 x 3 square with everything outside the image counting as 0, d = max(1,
round(dilation_ratio * sqrt(H^2 + W^2))) of the mask's OWN image.  A pair's boundary IoU is |Bd(d) & Bd(g)| / |Bd(d) | Bd(g)|, and
|Bd(d) & Bd(g)| / |Bd(d)| against a crowd (the crowd rule applied to the bands); the IoU that enters matching is min(mask IoU,
boundary IoU); areas stay mask areas.  Per chunk that is two more launches: the bands of all planes of all images, each with its
own size and d (csrc/mask_boundary.hip, erode_ragged_kernel), and the mask-IoU kernel a second time on the band buffer through the
same tables.  An image whose band is wider than 64 pixels (a diagonal above about 3200 px at ratio 0.02) takes the chained
per-image call instead.  Restated; parity with the boundary_iou package is unpinned.

    python -m s2d_amd.coco_eval --gt ann.json --results res.json [--iou-type segm|bbox|boundary] [--dilation-ratio 0.02] [--use-cats]
"""
import argparse
import itertools
import json
import logging
import os
import time
from collections import Counter, OrderedDict, defaultdict
from types import SimpleNamespace

import numpy as np

from .ytvis_eval import IOU_THRS, REC_THRS, YTVISEval, decode_staged, plane_bboxes, stage_rle

AREA_RNG = [[0, 1e10], [0, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e10]]
AREA_LBL = ["all", "small", "medium", "large"]
METRICS = ["AP", "AP50", "AP75", "APs", "APm", "APl", "AR1", "AR10", "AR100", "ARs", "ARm", "ARl"]
CHUNK_WORDS = 1 << 26          # plane words of one chunk (256 MiB): about 60 COCO-val images with 100 detections each.  The per-image
#                                planes are concatenated into the flat buffer the kernel reads, so the peak is about twice this.
#                                "boundary" keeps a third copy, the bands, and counts an image's words double against the limit: a
#                                chunk then holds half the words and the peak is 3 x half = about 1.5 times this (384 MiB)
CHUNK_IMAGES = 1024
LIB_CALLS = Counter()          # library calls made for this module, by export name ("decode": the per-image decode / bbox calls)

_log = logging.getLogger(__name__)


def _device(device):
    import torch
    return torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())


def _up(a, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev) if a.size else None


def _lib_call(name, *args):
    from ._lib import lib
    LIB_CALLS[name] += 1
    lib().call(name, *args)


def ragged_tables(Ds, Gs):
    """-> (dt0 [N+1], gt0 [N+1], pair0 [N+1]) int64: the flat numbering of a chunk (include/s2d_hip.h, "Ragged layout")"""
    Ds, Gs = np.asarray(Ds, np.int64).reshape(-1), np.asarray(Gs, np.int64).reshape(-1)
    z = np.zeros(1, np.int64)
    return np.concatenate([z, np.cumsum(Ds)]), np.concatenate([z, np.cumsum(Gs)]), np.concatenate([z, np.cumsum(Ds * Gs)])


def _image_table(Ds, Gs):
    dt0, gt0, pair0 = ragged_tables(Ds, Gs)
    img = np.zeros((len(Ds), 9), np.int64)
    img[:, 4], img[:, 5], img[:, 6], img[:, 7], img[:, 8] = Ds, Gs, dt0[:-1], gt0[:-1], pair0[:-1]
    return img, dt0, gt0, pair0


def chunk_tables(Ds, Gs, sizes):
    """the host tables of a chunk whose image n has Ds[n] + Gs[n] planes of sizes[n] = (H, W), back to back in one flat buffer (the D
    planes, then the G planes) -> (img int64 [N, 9], tiles int32 [n_tiles, 3], dt0, gt0, pair0, words): what
    s2d_coco_mask_iou_ragged reads (include/s2d_hip.h, "Ragged layout"; max(1, ceil(D/8)) * max(1, ceil(G/8)) pair tiles for every
    image with planes) and the buffer's length"""
    img, dt0, gt0, pair0 = _image_table(Ds, Gs)
    tiles, word = [], 0
    for n, (H, W) in enumerate(sizes):
        if H < 1 or W < 1 or H * W >= 1 << 31:
            raise ValueError(f"image of {H}x{W}")
        wpp = (H * W + 31) // 32
        D, G = int(img[n, 4]), int(img[n, 5])
        img[n, :4] = word, word + D * wpp, wpp, H * W
        word += (D + G) * wpp
        if D + G:
            ntd, ntg = max(1, (D + 7) // 8), max(1, (G + 7) // 8)
            tiles.append(np.stack([np.full(ntd * ntg, n), np.repeat(np.arange(ntd), ntg), np.tile(np.arange(ntg), ntd)], 1))
    tiles_h = np.concatenate(tiles).astype(np.int32) if tiles else np.zeros((0, 3), np.int32)
    return img, tiles_h, dt0, gt0, pair0, word


def staged_chunk(bits, Ds, Gs, sizes, crowd, dev):
    """-> the SimpleNamespace stage_planes documents, for a flat buffer `bits` (int32 CUDA [words], or None for a chunk without
    planes) that already holds the chunk's planes in the layout of chunk_tables; crowd: uint8 [sum Gs].  The tables are uploaded once."""
    img, tiles_h, dt0, gt0, pair0, word = chunk_tables(Ds, Gs, sizes)
    crowd_h = np.asarray(crowd, np.uint8).reshape(-1)
    if crowd_h.size != gt0[-1]:
        raise ValueError("crowd flags do not match the ground-truth planes")
    st = SimpleNamespace(bits=None, words=word, N=len(sizes), img=img, dt0=dt0, gt0=gt0, pair0=pair0, img_dev=None, tiles_dev=None,
                         n_tiles=0, crowd_dev=None, dev=dev)
    if len(tiles_h):
        if bits is None or bits.dim() != 1 or bits.numel() != word:
            raise ValueError(f"a buffer of {None if bits is None else tuple(bits.shape)} for a chunk of {word} words")
        st.bits = bits
        st.img_dev, st.tiles_dev, st.n_tiles, st.crowd_dev = _up(img, dev), _up(tiles_h, dev), len(tiles_h), _up(crowd_h, dev)
    return st


# --------------------------------------------------------------------------------------------------------------- device
def stage_planes(planes, crowd, device=None):
    """the chunk's planes concatenated ONCE into the flat buffer the kernels read, and the tables uploaded once (arguments as
    mask_iou_ragged's) -> SimpleNamespace(bits int32 CUDA [words] or None for a chunk without planes, words, N, img / dt0 / gt0 /
    pair0 host tables, img_dev, tiles_dev, n_tiles, crowd_dev, dev): what mask_iou_staged reads, on `bits` or on any buffer of
    the same layout (the boundary bands)"""
    import torch
    from . import ops
    dev = _device(device)
    Ds = [0 if p[0] is None else int(p[0].shape[0]) for p in planes]
    Gs = [0 if p[1] is None else int(p[1].shape[0]) for p in planes]
    parts = []
    for db, gb, H, W in planes:
        wpp = (H * W + 31) // 32
        if H < 1 or W < 1 or H * W >= 1 << 31:
            raise ValueError(f"image of {H}x{W}")
        for b in (db, gb):
            if b is not None:
                ops._chk(b, torch.int32)
                if b.dim() != 2 or b.shape[1] != wpp:
                    raise ValueError(f"planes of shape {tuple(b.shape)} for a {H}x{W} image ({wpp} words)")
                if b.shape[0]:
                    parts.append(b.reshape(-1))
    if len(crowd) != len(planes) or any(len(c) != g for c, g in zip(crowd, Gs)):
        raise ValueError("crowd flags do not match the ground-truth planes")
    crowd_h = np.concatenate([np.asarray(c, np.uint8).reshape(-1) for c in crowd]) if len(crowd) else np.zeros(0, np.uint8)
    bits = (torch.cat(parts) if len(parts) > 1 else parts[0]) if parts else None
    return staged_chunk(bits, Ds, Gs, [(p[2], p[3]) for p in planes], crowd_h, dev)


def mask_iou_staged(st, bits=None):
    """One launch (s2d_coco_mask_iou_ragged) on the staged chunk `st`, reading st.bits or `bits`, an int32 CUDA buffer of the same
    layout -> the SimpleNamespace mask_iou_ragged documents"""
    import torch
    from . import ops
    dev = st.dev
    out = SimpleNamespace(iou=torch.empty((int(st.pair0[-1]),), device=dev, dtype=torch.float64),
                          inter=torch.empty((int(st.pair0[-1]),), device=dev, dtype=torch.int64),
                          area_d=torch.empty((int(st.dt0[-1]),), device=dev, dtype=torch.int32),
                          area_g=torch.empty((int(st.gt0[-1]),), device=dev, dtype=torch.int32), img=st.img, dt0=st.dt0, gt0=st.gt0,
                          pair0=st.pair0)
    if st.n_tiles:
        bits = st.bits if bits is None else bits
        ops._chk(bits, torch.int32)
        if bits.dim() != 1 or bits.numel() != st.words or bits.device != st.bits.device:
            raise ValueError(f"a buffer of {tuple(bits.shape)} words for a chunk of {st.words}")
        _lib_call("s2d_coco_mask_iou_ragged", bits, st.img_dev, st.N, st.tiles_dev, st.n_tiles, st.crowd_dev,
                   out.inter, out.area_d, out.area_g, out.iou, ops._stream())
    return out


def mask_iou_ragged(planes, crowd, device=None):
    """planes: per image (dt_bits int32 CUDA [D, wpp] or None, gt_bits [G, wpp] or None, H, W) in the layout of
    ytvis_eval.decode_frames; crowd: per image the G crowd flags.  One launch (s2d_coco_mask_iou_ragged) ->
    SimpleNamespace(iou f64 CUDA [P], inter int64 CUDA [P], area_d / area_g int32 CUDA, img, dt0, gt0, pair0 host tables)"""
    return mask_iou_staged(stage_planes(planes, crowd, device))


def boundary_bands_ragged(bits, spec, out=None):
    """The boundary bands of a chunk's planes in one launch (s2d_mask_boundary_ragged_plan + s2d_mask_boundary_ragged_u32).
    bits: int32 CUDA [words], the flat buffer of stage_planes; spec: host int64 [N, 5] = {word0, F, H, W, d} per image (F planes of
    ceil(H*W/32) words from word0; F = 0: an image this call leaves out).  -> int32 CUDA [words] (`out` if given): every listed plane's
    band M & ~erode(M, d) at the plane's own offset, padding bits 0; words of no listed plane are 0 or untouched (include/s2d_hip.h).
    Every table entry is checked against the buffer before the launch; a clamped d above 64 is refused (boundary_planes chains)."""
    import torch
    from . import ops
    ops._chk(bits, torch.int32)
    if bits.dim() != 1:
        raise ValueError(f"boundary_bands_ragged: a flat buffer, not {tuple(bits.shape)}")
    spec = np.ascontiguousarray(spec, np.int64).reshape(-1, 5)
    N, words = len(spec), bits.numel()
    if N:
        word0, F, H, W, d = spec.T
        ok = (F >= 0).all() and (H >= 1).all() and (W >= 1).all() and (H < 1 << 31).all() and (W < 1 << 31).all() and (d >= 1).all()
        ok = ok and (H * W < 1 << 31).all() and (np.minimum(d, (np.minimum(H, W) + 1) // 2) <= 64).all()
        if ok:
            end = word0 + F * ((H * W + 31) // 32)
            ok = word0[0] >= 0 and (word0[1:] >= end[:-1]).all() and (end <= words).all() and (word0 <= words).all()
        if not ok:
            raise ValueError("boundary_bands_ragged: inconsistent tables")
    if out is None:
        out = torch.empty_like(bits)
    ops._chk(out, torch.int32)
    if out.shape != bits.shape or out.device != bits.device or out.data_ptr() == bits.data_ptr():
        raise ValueError("boundary_bands_ragged: out must be a second buffer of the same size on the same device")
    if N and words:
        plan, nwg, lds = np.zeros((N, 12), np.int64), np.zeros(1, np.int64), np.zeros(1, np.int64)
        _lib_call("s2d_mask_boundary_ragged_plan", spec, N, words, plan, nwg, lds)
        _lib_call("s2d_mask_boundary_ragged_u32", bits, words, plan, _up(plan, bits.device), N, out, ops._stream())
    return out


def box_iou_ragged(dt_boxes, gt_boxes, crowd, device=None):
    """per image float64 boxes [D, 4], [G, 4] ([x, y, w, h]) and G crowd flags -> SimpleNamespace(iou f64 CUDA [P], tables), one
    launch (s2d_coco_box_iou_ragged; maskApi.c bbIou)"""
    import torch
    from . import ops
    from ._lib import lib
    dev = _device(device)
    dt_boxes = [np.asarray(b, np.float64).reshape(-1, 4) for b in dt_boxes]
    gt_boxes = [np.asarray(b, np.float64).reshape(-1, 4) for b in gt_boxes]
    if not (len(dt_boxes) == len(gt_boxes) == len(crowd)) or any(len(c) != len(g) for c, g in zip(crowd, gt_boxes)):
        raise ValueError("box lists and crowd flags do not match")
    img, dt0, gt0, pair0 = _image_table([len(b) for b in dt_boxes], [len(b) for b in gt_boxes])
    out = SimpleNamespace(iou=torch.empty((int(pair0[-1]),), device=dev, dtype=torch.float64), img=img, dt0=dt0, gt0=gt0, pair0=pair0)
    if pair0[-1]:
        crowd_h = np.concatenate([np.asarray(c, np.uint8).reshape(-1) for c in crowd])
        _lib_call("s2d_coco_box_iou_ragged", _up(np.concatenate(dt_boxes), dev), _up(np.concatenate(gt_boxes), dev), _up(crowd_h, dev),
                   _up(img, dev), len(img), _up(pair0, dev), int(pair0[-1]), out.iou, ops._stream())
    return out


def match_ragged(iou, groups, dsel, gsel, dt_area, gt_area, gt_ignore, crowd, iou_thrs=IOU_THRS, area_rng=AREA_RNG):
    """evaluateImg of every group x area range x threshold in one launch (s2d_coco_match; tables as include/s2d_hip.h documents
    them: groups int64 [n, 8], dsel / gsel int32 flat numbers, dt_area / gt_area float64, gt_ignore / crowd uint8 per flat
    ground truth).  iou: the chunk's float64 CUDA IoU blocks.  -> numpy int32 (dt_match, gt_match, dt_ignore, gt_ignore, gt_perm)
    in the documented layouts.  Every table entry is checked against the array sizes before the launch."""
    import torch
    from . import ops
    from ._lib import lib
    ops._chk(iou, torch.float64)
    dev = iou.device
    groups = np.ascontiguousarray(groups, np.int64).reshape(-1, 8)
    dsel, gsel = np.ascontiguousarray(dsel, np.int32), np.ascontiguousarray(gsel, np.int32)
    dt_area, gt_area = np.ascontiguousarray(dt_area, np.float64), np.ascontiguousarray(gt_area, np.float64)
    gt_ignore, crowd = np.ascontiguousarray(gt_ignore, np.uint8), np.ascontiguousarray(crowd, np.uint8)
    thrs = np.ascontiguousarray(iou_thrs, np.float64)
    rng = np.ascontiguousarray(area_rng, np.float64).reshape(-1, 2)
    T, A, n = len(thrs), len(rng), len(groups)
    nd, ng = len(dsel), len(gsel)
    if n:
        pair0, ldg, dt0, gt0, ds0, D, gs0, G = groups.T
        ok = (D >= 0).all() and (G >= 0).all() and (ds0 == np.concatenate([[0], np.cumsum(D)[:-1]])).all() and D.sum() == nd \
            and (gs0 == np.concatenate([[0], np.cumsum(G)[:-1]])).all() and G.sum() == ng and len(gt_ignore) == len(crowd) == len(gt_area)
        if ok and nd:
            ok = dsel.min() >= 0 and dsel.max() < len(dt_area) and (dsel >= np.repeat(dt0, D)).all()
        if ok and ng:
            ok = gsel.min() >= 0 and gsel.max() < len(gt_area) and (gsel >= np.repeat(gt0, G)).all() \
                and (gsel - np.repeat(gt0, G) < np.repeat(ldg, G)).all()
        if ok and nd and ng:                                              # the last element a group can read lies inside iou
            has = (D > 0) & (G > 0)
            rmax = np.maximum.reduceat(dsel, ds0[D > 0])[has[D > 0]] - dt0[has]
            ok = (pair0[has] >= 0).all() and (pair0[has] + (rmax + 1) * ldg[has] <= iou.numel()).all()
        if not ok:
            raise ValueError("match_ragged: inconsistent tables")
    i32 = lambda k: torch.empty((k,), device=dev, dtype=torch.int32)      # noqa: E731
    dtm, gtm, dti, gti, gpm = i32(T * A * nd), i32(T * A * ng), i32(T * A * nd), i32(A * ng), i32(A * ng)
    if n:
        _lib_call("s2d_coco_match", iou if iou.numel() else None, _up(groups, dev), n, _up(dsel, dev), _up(gsel, dev), _up(dt_area, dev),
                   _up(gt_area, dev), _up(gt_ignore, dev), _up(crowd, dev), _up(thrs, dev), T, _up(rng, dev), A, dtm, gtm, dti, gti, gpm,
                   ops._stream())
    return tuple(t.cpu().numpy() for t in (dtm, gtm, dti, gti, gpm))


def decode_segmentations(segs, H, W, device=None):
    """COCO segmentations of one image -- RLE dicts (compressed or uncompressed) or polygon lists -- -> int32 CUDA bit planes
    [len(segs), ceil(H*W/32)]: the RLEs parsed and decoded on the device, the polygons rasterised into their rows"""
    from .data.image_clip import _valid_polygons, polygons_to_bits
    dev = _device(device)
    for s in segs:
        if not isinstance(s, (dict, list, tuple)):
            raise ValueError(f"no segmentation to decode: {s!r}")
    bits = decode_staged(stage_rle([s if isinstance(s, dict) else None for s in segs], H, W), H, W, dev)
    rows = [i for i, s in enumerate(segs) if not isinstance(s, dict)]
    if rows:
        polygons_to_bits([_valid_polygons(segs[i]) for i in rows], H, W, out=bits, rows=rows)
    # what the two wrappers above call: s2d_rle_parse_strings + s2d_rle_decode_bits for a non-empty list, s2d_polygons_to_bits if any
    LIB_CALLS["decode"] += (2 if len(segs) else 0) + (1 if rows else 0)
    return bits


# --------------------------------------------------------------------------------------------------------------- data
class COCOGroundTruth:
    """The parts of a COCO instances document the evaluation reads (COCO.createIndex + COCOeval._prepare): images, annotations
    per image in document order, sorted category ids"""

    def __init__(self, doc):
        if isinstance(doc, (str, os.PathLike)):
            with open(doc) as fh:
                doc = json.load(fh)
        if "images" not in doc:
            raise ValueError("not a COCO image document: no `images`")
        self.doc = doc
        self.images = {im["id"]: im for im in doc["images"]}
        self.cat_ids = sorted(c["id"] for c in doc.get("categories", []))
        self.img_ids = [int(i) for i in np.unique(list(self.images.keys()))] if self.images else []
        self.has_annotations = "annotations" in doc
        self.anns = defaultdict(list)                                  # image_id -> annotations in document order
        for a in doc.get("annotations", []):
            if a["image_id"] not in self.images:
                raise ValueError(f"annotation {a.get('id')} names image {a['image_id']}, which the document does not have")
            self.anns[a["image_id"]].append(a)

    def image(self, iid):
        return self.images[iid]

    def gts(self, iid):
        """per ground truth of the image: id, category, crowd flag, ignore (= iscrowd), the annotation's own `area` and `bbox`
        (None where absent: evaluate_coco fills them from the mask), segmentation"""
        out = []
        for a in self.anns.get(iid, []):
            crowd = int(a.get("iscrowd", 0))
            out.append(SimpleNamespace(id=a["id"], category_id=a["category_id"], iscrowd=crowd, ignore=bool(crowd),
                                       area=a.get("area"), avg_area=a.get("area"), bbox=a.get("bbox"), segmentation=a.get("segmentation")))
        return out


# --------------------------------------------------------------------------------------------------------------- host
class COCOEval(YTVISEval):
    """Matching, accumulation and summary of COCOeval on per-image IoU matrices.

    `evaluate(images)` takes, per image id, {"dt_ids", "scores", "labels", "areas", "ious"}: the detections in result order and
    their IoU against every ground truth of the image in document order ([D, G]); ground truths come from `gt.gts` and must have
    an area (`gt_areas` {image id: [G]} overrides / supplies them).  matcher="device": s2d_coco_match, one launch for all of
    `images`; matcher="host": YTVISEval._evaluate_video's Python loop on the same matrices.  Attributes as YTVISEval's:
    `eval_imgs` (= `eval_vids`, the evaluateImg dicts in category, area range, image order, None where an image has neither),
    `eval["precision"]` [T,R,K,A,M], `eval["recall"]` [T,K,A,M], `stats` (12)."""

    def __init__(self, gt, iou_type="segm", use_cats=False, max_dets=(1, 10, 100)):
        self.gt = gt if isinstance(gt, COCOGroundTruth) else COCOGroundTruth(gt)
        ids = list(self.gt.img_ids)
        self.params = SimpleNamespace(imgIds=ids, vidIds=ids, catIds=list(self.gt.cat_ids), iouThrs=IOU_THRS, recThrs=REC_THRS,
                                      maxDets=sorted(max_dets), areaRng=AREA_RNG, areaRngLbl=AREA_LBL, useCats=int(bool(use_cats)),
                                      iouType=iou_type)
        # accumulate() and _summarize_one() are YTVISEval's and read ytvis_eval's own AREA_RNG (for its length) and AREA_LBL, not
        # self.params: the two tables must keep the same number of ranges and the same labels
        from . import ytvis_eval
        assert len(AREA_RNG) == len(ytvis_eval.AREA_RNG) and AREA_LBL == ytvis_eval.AREA_LBL
        self.ious, self.eval_vids, self.eval, self.stats = {}, [], {}, []
        self._cells = {}
        self.launches = defaultdict(int)
        self.seconds = defaultdict(float)

    @property
    def eval_imgs(self):
        return self.eval_vids

    # one chunk: images -> self._cells[(image, category, area index)] -----------------------------------------------------
    def _prepare(self, img_ids, images, gt_areas):
        p = self.params
        cats = p.catIds if p.useCats else [-1]
        chunk = []
        for iid in img_ids:
            gts = self.gt.gts(iid)
            if gt_areas is not None and iid in gt_areas:
                for g, a in zip(gts, gt_areas[iid]):
                    g.area = g.avg_area = a
            for g in gts:
                if g.area is None:
                    raise ValueError(f"ground truth {g.id} of image {iid} has no area")
            v = images.get(iid)
            if v is None:
                v = {"dt_ids": [], "scores": [], "labels": [], "areas": [], "ious": np.zeros((0, len(gts)))}
            D = len(v["scores"])
            ious = np.asarray(v["ious"], np.float64).reshape(D, len(gts))
            gcat = [g.category_id for g in gts]
            groups = []
            for cat in cats:
                gi = self._group(gcat, cat)
                di = self._group(list(v["labels"]), cat)
                order = np.argsort([-v["scores"][i] for i in di], kind="mergesort")
                di = [di[i] for i in order][:p.maxDets[-1]]
                if gi or di:
                    self.ious[iid, cat] = ious[np.ix_(np.asarray(di, np.intp), np.asarray(gi, np.intp))]
                else:
                    self.ious[iid, cat] = []
                groups.append((cat, di, gi))
            chunk.append(SimpleNamespace(iid=iid, gts=gts, v=v, D=D, G=len(gts), ious=ious, groups=groups))
        return chunk

    def _match_host(self, chunk):
        p = self.params
        for im in chunk:
            for cat, di, gi in im.groups:
                self._gts[im.iid, cat] = [im.gts[i] for i in gi]
                self._dts[im.iid, cat] = [SimpleNamespace(id=im.v["dt_ids"][i], score=im.v["scores"][i], avg_area=im.v["areas"][i]) for i in di]
                for a, rng in enumerate(p.areaRng):
                    e = self._evaluate_video(im.iid, cat, rng, p.maxDets[-1])
                    if e is not None:
                        e["image_id"] = e.pop("video_id")
                    self._cells[im.iid, cat, a] = e
                del self._gts[im.iid, cat], self._dts[im.iid, cat]

    def _match_device(self, chunk, iou_dev, device):
        import torch
        p = self.params
        A, T = len(p.areaRng), len(IOU_THRS)
        dt0, gt0, pair0 = ragged_tables([im.D for im in chunk], [im.G for im in chunk])
        if iou_dev is None:
            flat = np.concatenate([im.ious.reshape(-1) for im in chunk]) if chunk else np.zeros(0)
            iou_dev = torch.from_numpy(np.ascontiguousarray(flat, np.float64)).to(_device(device))
        rows, dsel, gsel, where = [], [], [], []
        nd = ng = 0
        for n, im in enumerate(chunk):
            for cat, di, gi in im.groups:
                if not (gi or di):
                    for a in range(A):
                        self._cells[im.iid, cat, a] = None
                    continue
                rows.append([pair0[n], im.G, dt0[n], gt0[n], nd, len(di), ng, len(gi)])
                dsel += [dt0[n] + i for i in di]
                gsel += [gt0[n] + i for i in gi]
                where.append((im, cat, di, gi, nd, ng))
                nd, ng = nd + len(di), ng + len(gi)
        flat_g = [g for im in chunk for g in im.gts]
        before = LIB_CALLS["s2d_coco_match"]
        dtm, gtm, dti, gti, gpm = match_ragged(
            iou_dev, np.asarray(rows, np.int64).reshape(-1, 8), dsel, gsel, [a for im in chunk for a in im.v["areas"]],
            [g.area for g in flat_g], [g.ignore for g in flat_g], [g.iscrowd for g in flat_g], IOU_THRS, p.areaRng)
        self.launches["match"] += LIB_CALLS["s2d_coco_match"] - before
        for im, cat, di, gi, d0, g0 in where:
            D, G = len(di), len(gi)
            dt_ids = np.asarray([im.v["dt_ids"][i] for i in di], np.float64)
            scores = [im.v["scores"][i] for i in di]
            for a, rng in enumerate(p.areaRng):
                gb, db = A * g0 + a * G, A * d0 + a * D
                perm = gpm[gb:gb + G]
                gt_ids = np.asarray([im.gts[gi[k]].id for k in perm], np.float64)
                dm = dtm[T * db:T * (db + D)].reshape(T, D)
                gm = gtm[T * gb:T * (gb + G)].reshape(T, G)
                self._cells[im.iid, cat, a] = {
                    "image_id": im.iid, "category_id": cat, "aRng": rng, "maxDet": p.maxDets[-1], "dtIds": [int(i) for i in dt_ids],
                    "gtIds": [im.gts[gi[k]].id for k in perm],
                    "dtMatches": np.where(dm >= 0, gt_ids[np.maximum(dm, 0)], 0.0) if G else np.zeros((T, D)),
                    "gtMatches": np.where(gm >= 0, dt_ids[np.maximum(gm, 0)], 0.0) if D else np.zeros((T, G)),
                    "dtScores": scores, "gtIgnore": gti[gb:gb + G].astype(np.int64), "dtIgnore": dti[T * db:T * (db + D)].reshape(T, D) != 0}

    def add_chunk(self, img_ids, images, matcher="device", gt_areas=None, iou_dev=None, device=None):
        """match one chunk of images (ids of the ground truth, each at most once over all chunks)"""
        if matcher not in ("device", "host"):
            raise ValueError(f"matcher {matcher!r}: 'device' or 'host'")
        chunk = self._prepare(img_ids, images, gt_areas)
        if matcher == "host":
            self._gts, self._dts = {}, {}
            self._match_host(chunk)
        else:
            self._match_device(chunk, iou_dev, device)

    def finish(self):
        p = self.params
        cats = p.catIds if p.useCats else [-1]
        self.eval_vids = [self._cells.get((iid, cat, a)) for cat in cats for a in range(len(p.areaRng)) for iid in p.imgIds]
        return self

    def evaluate(self, images, matcher="device", gt_areas=None, device=None):
        for iid in images:
            if iid not in self.gt.images:
                raise ValueError(f"results for image {iid}, which the ground truth does not have")
        self.add_chunk(self.params.imgIds, images, matcher, gt_areas, device=device)
        return self.finish()

    def accumulate(self):
        t0 = time.perf_counter()
        super().accumulate()
        self.seconds["accumulate"] += time.perf_counter() - t0
        return self


def derive_results(stats):
    """the 12 named metrics x 100, nan where the stat is -1 (detectron2 COCOEvaluator._derive_coco_results)"""
    return {m: float(stats[i] * 100 if stats[i] >= 0 else "nan") for i, m in enumerate(METRICS)}


def _box_area(boxes):
    return boxes[:, 2] * boxes[:, 3]


def evaluate_coco(gt, results, *, iou_type="segm", use_cats=False, max_dets=(1, 10, 100), device=None, matcher="device",
                  profile=False, dilation_ratio=0.02):
    """Score a COCO results list / file ({image_id, category_id, score, segmentation and/or bbox}) against a COCO instances
    document / file.  Returns the COCOEval after evaluate + accumulate (call .summarize() for the table and .stats).
    matcher="host": the Python matching loop on the device-computed IoUs (reference path).  profile: synchronise between the
    phases so that `.seconds` (decode, iou, match, accumulate) are device-inclusive times; `.launches` counts the library calls made ("decode": RLE parse,
    RLE decode, polygon fill and plane-bbox calls, per image; "iou" and "match": one per non-empty chunk) either way.
    iou_type="boundary": Boundary AP -- matching on min(mask IoU, boundary IoU), the bands `dilation_ratio` of each image's
    diagonal wide; `.seconds["boundary"]` is the band phase, `.launches["boundary"]` the ragged band calls (one per non-empty chunk),
    `.launches["boundary_chained"]` the images whose band is wider than 64 pixels and goes through boundary_planes, and
    `.launches["iou"]` is 2 per non-empty chunk (masks, bands)."""
    import torch
    from .ytvis_eval import boundary_dilation, boundary_planes
    if iou_type not in ("segm", "bbox", "boundary"):
        raise ValueError(f"iou_type {iou_type!r}: 'segm', 'bbox' or 'boundary'")
    if isinstance(results, (str, os.PathLike)):
        with open(results) as fh:
            results = json.load(fh)
    gt = gt if isinstance(gt, COCOGroundTruth) else COCOGroundTruth(gt)
    dev = _device(device)
    by_img = defaultdict(list)
    for n, r in enumerate(results):
        if r["image_id"] not in gt.images:
            raise ValueError(f"results for image {r['image_id']}, which the ground truth does not have")
        by_img[r["image_id"]].append(n)
    ev = COCOEval(gt, iou_type, use_cats, max_dets)
    boundary = iou_type == "boundary"
    segm = iou_type == "segm" or boundary

    def tick(name, t0):
        if profile:
            torch.cuda.synchronize(dev)
        ev.seconds[name] += time.perf_counter() - t0

    def plan(iid):
        im = gt.image(iid)
        idx = by_img.get(iid, [])
        gts = gt.gts(iid)
        dsegs, gsegs = [results[n].get("segmentation") for n in idx], [g.segmentation for g in gts]
        dbox, gbox = [results[n].get("bbox") for n in idx], [g.bbox for g in gts]
        entries = list(zip(dsegs + gsegs, dbox + gbox))
        if any(s is None for s, _ in entries) if segm else any(s is None and b is None for s, b in entries):
            raise ValueError(f"image {iid}: a result or annotation without a segmentation" + ("" if segm else " or bbox"))
        need = list(range(len(entries))) if segm else [k for k, (_, b) in enumerate(entries) if b is None]     # planes to decode
        words = len(need) * ((im["height"] * im["width"] + 31) // 32) * (2 if boundary else 1)        # the bands are a copy more
        return SimpleNamespace(iid=iid, H=im["height"], W=im["width"], idx=idx, gts=gts, dsegs=dsegs, gsegs=gsegs, dbox=dbox, gbox=gbox,
                               need=need, words=words)

    def bands(chunk, st):
        """the chunk's boundary bands in the layout of st.bits: one ragged call, and boundary_planes for an image whose band is
        wider than one pass takes (written after the ragged call, which may zero the whole buffer)"""
        spec, chained = np.zeros((len(chunk), 5), np.int64), []
        for n, c in enumerate(chunk):
            d = boundary_dilation(c.H, c.W, dilation_ratio)
            one_pass = min(d, (min(c.H, c.W) + 1) // 2) <= 64
            F = int(st.img[n, 4] + st.img[n, 5])
            spec[n] = st.img[n, 0], F if one_pass else 0, c.H, c.W, d if one_pass else 1
            if F and not one_pass:
                chained.append((n, c, d))
        before = LIB_CALLS["s2d_mask_boundary_ragged_u32"]
        band = boundary_bands_ragged(st.bits, spec)
        ev.launches["boundary"] += LIB_CALLS["s2d_mask_boundary_ragged_u32"] - before
        for n, c, d in chained:
            w0 = int(st.img[n, 0])
            band[w0:w0 + c.bits.numel()] = boundary_planes(c.bits, c.H, c.W, d).reshape(-1)
            ev.launches["boundary_chained"] += 1
        return band

    def run(chunk):
        t0 = time.perf_counter()
        before = LIB_CALLS["decode"]
        for c in chunk:                                                   # decode: per image (its own size)
            segs = c.dsegs + c.gsegs
            c.bits = decode_segmentations([segs[k] for k in c.need], c.H, c.W, dev) if c.need else None
        tick("decode", t0)
        t0 = time.perf_counter()
        crowd = [[g.iscrowd for g in c.gts] for c in chunk]
        calls = LIB_CALLS["s2d_coco_mask_iou_ragged"] + LIB_CALLS["s2d_coco_box_iou_ragged"]
        if segm:
            D = [len(c.idx) for c in chunk]
            st = stage_planes([(c.bits[:d] if c.bits is not None else None, c.bits[d:] if c.bits is not None else None, c.H, c.W)
                               for c, d in zip(chunk, D)], crowd, dev)
            r = mask_iou_staged(st)
            if boundary and st.bits is not None:
                tick("iou", t0)
                t0 = time.perf_counter()
                r.iou = torch.minimum(r.iou, mask_iou_staged(st, bands(chunk, st)).iou)
                tick("boundary", t0)              # the band IoU launch and the min are booked here: "iou" stays what "segm" spends
                t0 = time.perf_counter()
            d_area, g_pix = r.area_d.cpu().numpy().astype(np.float64), r.area_g.cpu().numpy()
        else:
            boxes = []
            for c in chunk:                                               # only the box-less entries were decoded: their tight boxes
                b = np.array([[0.0] * 4 if g is None else g for g in c.dbox + c.gbox], np.float64).reshape(-1, 4)
                if c.need:
                    b[c.need] = plane_bboxes(c.bits, c.H, c.W).cpu().numpy()
                    LIB_CALLS["decode"] += 1
                boxes.append(b)
            r = box_iou_ragged([b[:len(c.idx)] for b, c in zip(boxes, chunk)], [b[len(c.idx):] for b, c in zip(boxes, chunk)], crowd, dev)
            d_area = np.concatenate([_box_area(b[:len(c.idx)]) for b, c in zip(boxes, chunk)]) if chunk else np.zeros(0)
            g_pix = np.concatenate([_box_area(b[len(c.idx):]) for b, c in zip(boxes, chunk)]) if chunk else np.zeros(0)
        ev.launches["decode"] += LIB_CALLS["decode"] - before
        ev.launches["iou"] += LIB_CALLS["s2d_coco_mask_iou_ragged"] + LIB_CALLS["s2d_coco_box_iou_ragged"] - calls
        ious = r.iou.cpu().numpy()
        tick("iou", t0)
        images, gt_areas = {}, {}
        for n, c in enumerate(chunk):
            D, G = len(c.idx), len(c.gts)
            images[c.iid] = {"dt_ids": [k + 1 for k in c.idx], "scores": [results[k]["score"] for k in c.idx],
                             "labels": [results[k]["category_id"] for k in c.idx], "areas": d_area[r.dt0[n]:r.dt0[n + 1]].tolist(),
                             "ious": ious[r.pair0[n]:r.pair0[n + 1]].reshape(D, G)}
            gt_areas[c.iid] = [g.area if g.area is not None else g_pix[r.gt0[n] + j].item() for j, g in enumerate(c.gts)]
        t0 = time.perf_counter()
        ev.add_chunk([c.iid for c in chunk], images, matcher, gt_areas, iou_dev=r.iou, device=dev)
        tick("match", t0)

    chunk, words = [], 0
    for iid in ev.params.imgIds:
        c = plan(iid)
        if chunk and (words + c.words > CHUNK_WORDS or len(chunk) >= CHUNK_IMAGES):
            run(chunk)
            chunk, words = [], 0
        chunk.append(c)
        words += c.words
    if chunk:
        run(chunk)
    return ev.finish().accumulate()


class COCOImageEvaluator:
    """The image-side YTVISEvaluator (detectron2's COCOEvaluator protocol): `process(inputs, outputs)` takes one image's model
    output -- what inference_video returns for the one-frame video, masks as COCO RLE (inference_rle), as a CUDA u8 / bool
    tensor [K,1,H,W] or as CPU bool tensors -- and keeps its results entries; `evaluate()` gathers the ranks' entries, orders
    them by the ground truth's image order, writes output_dir/coco_instances_results.json and returns {"segm": {...},
    "bbox": {...}} (12 metrics x 100 each; the boxes are the tight boxes of the masks).  On a document without `annotations`
    it only writes the results.  Categories are pooled (use_cats=False), as in evaluate_ytvis.  iou_types may also hold
    "boundary" (opt-in): Boundary AP with bands `dilation_ratio` of the image diagonal wide, a dict of the same 12 names."""

    def __init__(self, json_file=None, output_dir=None, distributed=True, iou_types=("segm", "bbox"), dataset_id_to_contiguous_id=None,
                 dilation_ratio=0.02):
        if json_file is None:
            raise ValueError("COCOImageEvaluator needs json_file= (a path or a loaded document)")
        for t in iou_types:
            if t not in ("segm", "bbox", "boundary"):
                raise ValueError(f"iou type {t!r}: 'segm', 'bbox' or 'boundary'")
        self._distributed, self._output_dir, self._iou_types = distributed, output_dir, tuple(iou_types)
        self._dilation_ratio = dilation_ratio
        self._gt = COCOGroundTruth(json_file)
        self._do_evaluation = self._gt.has_annotations
        self._reverse = None
        if dataset_id_to_contiguous_id:
            ids = list(dataset_id_to_contiguous_id.values())
            assert min(ids) == 0 and max(ids) == len(ids) - 1
            self._reverse = {v: k for k, v in dataset_id_to_contiguous_id.items()}
        self.coco_eval = {}
        self.reset()

    def reset(self):
        self._records = []

    def process(self, inputs, outputs):
        import torch
        assert len(inputs) == 1, "More than one inputs are loaded for inference!"
        iid = inputs[0]["image_id"]
        if iid not in self._gt.images:
            raise ValueError(f"image {iid} is not in the ground truth")
        scores = [float(s) for s in outputs["pred_scores"]]
        labels = [int(l) for l in outputs["pred_labels"]]
        if self._reverse is not None:
            for l in labels:
                assert l < len(self._reverse), f"A prediction has class={l}, but the dataset only has {len(self._reverse)} classes"
            labels = [self._reverse[l] for l in labels]
        masks = outputs["pred_masks"]
        if scores and not (outputs.get("pred_masks_format") == "coco_rle" or isinstance(masks[0], (list, tuple))):
            from .rle import encode_video_predictions
            md = masks if isinstance(masks, torch.Tensor) else torch.stack([torch.as_tensor(m) for m in masks])
            md = md.view(torch.uint8) if md.dtype == torch.bool else md
            masks = encode_video_predictions(md.to(_device(None)).contiguous())
        for s, l, m in zip(scores, labels, masks):
            if len(m) != 1:
                raise ValueError(f"image {iid}: a prediction of {len(m)} frames")
            seg = dict(m[0], counts=m[0]["counts"].decode() if isinstance(m[0]["counts"], bytes) else m[0]["counts"])
            self._records.append({"image_id": iid, "category_id": l, "score": s, "segmentation": seg})

    def _gather(self):
        import torch.distributed as dist
        if self._distributed and dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            parts = [None] * dist.get_world_size()
            dist.all_gather_object(parts, self._records)
            if dist.get_rank() != 0:
                return None
            records = list(itertools.chain(*parts))
        else:
            records = list(self._records)
        pos = {im["id"]: n for n, im in enumerate(self._gt.doc["images"])}
        return sorted(records, key=lambda r: pos[r["image_id"]])         # stable: an image's entries keep their order

    def evaluate(self):
        records = self._gather()
        if records is None:
            return {}
        if not records:
            _log.warning("[COCOImageEvaluator] Did not receive valid predictions.")
            return {}
        if self._output_dir:
            os.makedirs(self._output_dir, exist_ok=True)
            with open(os.path.join(self._output_dir, "coco_instances_results.json"), "w") as fh:
                fh.write(json.dumps(records))
        results = OrderedDict()
        if not self._do_evaluation:
            _log.info("Annotations are not available for evaluation.")
            return results
        for t in self._iou_types:
            ev = evaluate_coco(self._gt, records, iou_type=t, dilation_ratio=self._dilation_ratio)
            ev.summarize()
            self.coco_eval[t] = ev
            results[t] = derive_results(ev.stats)
        return results


def main(argv=None):
    ap = argparse.ArgumentParser(description="COCO image mask / box AP and AR of a results file")
    ap.add_argument("--gt", required=True, help="COCO instances JSON")
    ap.add_argument("--results", required=True, help="results JSON (list of {image_id, category_id, score, segmentation and/or bbox})")
    ap.add_argument("--iou-type", choices=("segm", "bbox", "boundary"), default="segm")
    ap.add_argument("--dilation-ratio", type=float, default=0.02, help="boundary band width as a fraction of the image diagonal")
    ap.add_argument("--use-cats", action="store_true", help="per-category matching (the stock COCO protocol); default pools categories")
    a = ap.parse_args(argv)
    evaluate_coco(a.gt, a.results, iou_type=a.iou_type, use_cats=a.use_cats, dilation_ratio=a.dilation_ratio).summarize()


if __name__ == "__main__":
    main()
