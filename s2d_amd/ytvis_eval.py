"""YouTube-VIS video-instance evaluation (mask AP / AR): the reference's YTVISEvaluator
(model_training/mask2former_video/data_video/ytvis_eval.py) and its vendored YTVOS / YTVOSeval
(data_video/datasets/ytvis_api/ytvos.py, ytvoseval.py), without pycocotools and without masks on the host.

A pair's video IoU (ytvoseval.py:176-222) is  sum_t |d_t & g_t| / sum_t |d_t | g_t|  with an absent frame counting as an
empty plane, so it is exact from integers: the cross intersection counts of the two tracks and each track's area sum.  Those
come from the kernels of csrc/ytvis_eval.hip (RLE -> bit planes, cross popcounts, plane areas); predictions already on the
device are packed with s2d_pack_mask_bits_u8.  What is kept per video is small: the IoU matrix against the video's ground
truth, and the scores, categories and mean areas of its detections.

The greedy matching, `accumulate` and `summarize` run on the host in numpy (per video O(10 D G); the accumulate sort is over all
detections) with the reference's float operations, sort kinds and -1 sentinels, so `stats` come out identical.

Boundary AP (opt-in: iou_type="boundary" / boundary=True) scores contour quality, which mask IoU is nearly blind to on large
objects: Cheng et al., "Boundary IoU" (CVPR 2021) and the published mask_to_boundary routine, restated.  A mask's boundary band
is Bd = M & ~E, E = M eroded d times by a 3 x 3 square with everything outside the image counting as 0 (so mask pixels
within d of the image edge are boundary), d = max(1, round(dilation_ratio * sqrt(H^2 + W^2))) (csrc/mask_boundary.hip).  A
pair's video boundary IoU is  sum_t |Bd(d_t) & Bd(g_t)| / sum_t |Bd(d_t) | Bd(g_t)|,  the rule of the video mask IoU on the
bands and exact from the same three integer quantities; the IoU that enters matching is min(mask IoU, boundary IoU), and areas
stay mask areas.  The video form and the min rule are restated from the paper, not pinned against the boundary_iou package.

    python -m s2d_amd.ytvis_eval --gt ann.json --results results.json [--use-cats] [--iou-type boundary] [--dilation-ratio 0.02]
"""
import argparse
import itertools
import json
import logging
import os
from collections import OrderedDict, defaultdict
from types import SimpleNamespace

import numpy as np

IOU_THRS = np.linspace(.5, 0.95, int(np.round((0.95 - .5) / .05)) + 1, endpoint=True)
REC_THRS = np.linspace(.0, 1.00, int(np.round((1.00 - .0) / .01)) + 1, endpoint=True)
AREA_RNG = [[0 ** 2, 1e5 ** 2], [0 ** 2, 128 ** 2], [128 ** 2, 256 ** 2], [256 ** 2, 1e5 ** 2]]   # video areas: per-frame mean
AREA_LBL = ["all", "small", "medium", "large"]
METRICS = ["AP", "AP50", "AP75", "APs", "APm", "APl", "AR1", "AR10", "AR100"]

_log = logging.getLogger(__name__)


def mean_area(areas):
    """`avg_area` of ytvos.py / ytvoseval.py: mean of the truthy per-frame areas (None and 0 dropped), 0 if none remain"""
    kept = [a for a in areas if a]
    return np.array(kept).mean() if kept else 0


def _frame_kind(seg):
    if not seg:
        return None
    if isinstance(seg, list):
        raise NotImplementedError("polygon segmentations are not supported by the YTVIS evaluator: convert them to RLE")
    return "u" if isinstance(seg["counts"], list) else "c"


# --------------------------------------------------------------------------------------------------------------- device
def stage_rle(segs, H, W):
    """the host staging of decode_frames: COCO RLE frames (compressed dicts, uncompressed dicts, or None) of size [H, W] ->
    (chars u8, str_off int64 [F+1], ends int32, nrun int32 [F]) as numpy arrays, the inputs of s2d_rle_parse_strings /
    s2d_rle_decode_bits.  Uncompressed counts only get their running sums here; compressed strings are parsed on the device."""
    F, hw = len(segs), H * W
    lens = np.zeros(F, np.int64)
    nrun = np.zeros(F, np.int32)
    chunks, unc = [], {}
    for f, s in enumerate(segs):
        kind = _frame_kind(s)
        if kind is None:
            chunks.append(b"")
            continue
        if [int(v) for v in s["size"]] != [H, W]:
            raise ValueError(f"RLE of size {s['size']} in a video of size {[H, W]}")
        if kind == "c":
            c = s["counts"]
            c = c.encode() if isinstance(c, str) else bytes(c)
            chunks.append(c)
            lens[f] = len(c)
            nrun[f] = -1                                              # parsed on the device
        else:
            ends = np.minimum(np.cumsum(np.asarray(s["counts"], np.int64)), hw)
            chunks.append(bytes(len(ends)))                           # slots only: ends are written below
            lens[f] = nrun[f] = len(ends)
            unc[f] = ends
    str_off = np.zeros(F + 1, np.int64)
    np.cumsum(lens, out=str_off[1:])
    total = max(int(str_off[-1]), 1)
    chars = np.zeros(total, np.uint8)
    buf = b"".join(chunks)
    chars[:len(buf)] = np.frombuffer(buf, np.uint8)
    ends_h = np.zeros(total, np.int32)
    for f, e in unc.items():
        ends_h[str_off[f]:str_off[f] + len(e)] = e
    return chars, str_off, ends_h, nrun


def decode_staged(staged, H, W, dev, pinned=False):
    """stage_rle's arrays -> int32 CUDA bit planes [F, ceil(H*W/32)] on the current stream.  pinned: the copies go up from
    pinned memory without blocking the host (a loader's side stream)"""
    import torch
    from . import ops
    from ._lib import lib
    chars, str_off, ends_h, nrun = staged
    F = len(nrun)
    bits = torch.empty((F, (H * W + 31) // 32), device=dev, dtype=torch.int32)
    if F == 0:
        return bits
    up = (lambda a: torch.from_numpy(a).pin_memory().to(dev, non_blocking=True)) if pinned else (lambda a: torch.from_numpy(a).to(dev))
    chars_d, off_d, ends_d, nrun_d = up(chars), up(str_off), up(ends_h), up(nrun)
    st = ops._stream()
    lib().call("s2d_rle_parse_strings", chars_d, off_d, F, H * W, ends_d, nrun_d, st)
    lib().call("s2d_rle_decode_bits", ends_d, off_d, nrun_d, F, H, W, bits, st)
    return bits


def decode_frames(segs, H, W, device=None):
    """COCO RLE frames (compressed dicts, uncompressed dicts, or None for an absent frame), all of size [H, W] -> int32 CUDA
    bit planes [F, ceil(H*W/32)] (row-major flat index i -> word i/32, bit i%32).  Strings are parsed and every plane decoded
    on the device (s2d_rle_parse_strings, s2d_rle_decode_bits); uncompressed counts only get their running sums here."""
    import torch
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    return decode_staged(stage_rle(segs, H, W), H, W, dev)


def plane_areas(bits):
    """int32 CUDA bit planes [F, words] -> int32 CUDA [F] set pixels per plane"""
    import torch
    from . import ops
    from ._lib import lib
    ops._chk(bits, torch.int32)
    F, words = bits.shape
    area = torch.empty((F,), device=bits.device, dtype=torch.int32)
    if F:
        lib().call("s2d_mask_plane_areas_u32", bits, F, words, area, ops._stream())
    return area


def plane_bboxes(bits, H, W):
    """int32 CUDA bit planes [F, ceil(H*W/32)] -> int32 CUDA [F, 4]: x, y, w, h per plane, pycocotools rleToBbox
    (mask_util.toBbox) semantics; 0, 0, 0, 0 for an empty plane (s2d_mask_plane_bbox_u32)"""
    import torch
    from . import ops
    from ._lib import lib
    ops._chk(bits, torch.int32)
    F, words = bits.shape
    bbox = torch.empty((F, 4), device=bits.device, dtype=torch.int32)
    if F:
        lib().call("s2d_mask_plane_bbox_u32", bits, F, H, W, words, bbox, ops._stream())
    return bbox


def cross_counts(a, b):
    """int32 CUDA tracks a [D, words], b [G, words] -> int64 CUDA [D, G]: sum of popcount(a[d] & b[g])"""
    import torch
    from . import ops
    from ._lib import lib
    ops._chk(a, torch.int32); ops._chk(b, torch.int32)
    if a.shape[1] != b.shape[1]:
        raise ValueError(f"tracks of {a.shape[1]} and {b.shape[1]} words")
    inter = torch.zeros((a.shape[0], b.shape[0]), device=a.device, dtype=torch.int64)
    if a.shape[0] and b.shape[0]:
        lib().call("s2d_mask_cross_counts_u64", a, a.shape[0], b, b.shape[0], a.shape[1], inter, ops._stream())
    return inter


def boundary_dilation(H, W, ratio=0.02):
    """the erosion count of mask_to_boundary for an H x W image: max(1, round(ratio * image diagonal)), Python's round"""
    return max(1, int(round(ratio * np.sqrt(H * H + W * W))))


def boundary_planes(bits, H, W, d):
    """int32 CUDA bit planes [F, ceil(H*W/32)] -> their boundary bands M & ~erode(M, d) in the same layout, padding bits 0
    (s2d_mask_boundary_bits_u32)"""
    import torch
    from . import ops
    from ._lib import lib
    ops._chk(bits, torch.int32)
    F, words = bits.shape
    if words != (H * W + 31) // 32:
        raise ValueError(f"planes of {words} words for a {H}x{W} image")
    out = torch.empty_like(bits)
    if F:
        n = lib().call("s2d_mask_boundary_workspace_words", F, H, W, d)
        if n < 0:
            raise ValueError(f"boundary planes: F={F}, H={H}, W={W}, d={d} refused")
        ws = torch.empty((n,), device=bits.device, dtype=torch.int32) if n else None
        lib().call("s2d_mask_boundary_bits_u32", bits, F, H, W, d, ws, n, out, ops._stream())
    return out


def _track_ious(dt_bits, D, gt_bits, G, T):
    """-> (ious float64 [D, G], frame areas int64 [D, T]) from the planes' integer sums"""
    wpf = dt_bits.shape[1] if D else gt_bits.shape[1]
    d_area = plane_areas(dt_bits) if D else None
    g_area = plane_areas(gt_bits) if G else None
    inter = cross_counts(dt_bits.view(D, T * wpf), gt_bits.view(G, T * wpf)) if D and G else None
    da = d_area.cpu().numpy().astype(np.int64).reshape(D, T) if D else np.zeros((0, T), np.int64)
    ga = g_area.cpu().numpy().astype(np.int64).reshape(G, T) if G else np.zeros((0, T), np.int64)
    if inter is None:
        return np.zeros((D, G)), da
    i = inter.cpu().numpy()
    u = da.sum(1)[:, None] + ga.sum(1)[None, :] - i
    ious = np.zeros((D, G))
    pos = u > 0
    ious[pos] = i[pos] / u[pos]
    return ious, da


def video_ious(dt_bits, D, gt_bits, G, T, boundary_d=None, size=None):
    """bit planes of D detection and G ground-truth tracks ([D*T, wpf], [G*T, wpf], frames of a track adjacent) ->
    (ious float64 [D, G], detection frame areas int64 [D, T]).  iou = i / u in float64 from exact integer sums, 0 if u == 0.
    boundary_d (with size = (H, W)): -> (ious, areas, boundary ious float64 [D, G]), the same quotient on the planes'
    boundary bands at dilation boundary_d; the areas stay those of the masks."""
    ious, da = _track_ious(dt_bits, D, gt_bits, G, T)
    if boundary_d is None:
        return ious, da
    if size is None:
        raise ValueError("boundary_d needs size=(H, W)")
    if not (D and G):
        return ious, da, np.zeros((D, G))
    H, W = size
    bious, _ = _track_ious(boundary_planes(dt_bits, H, W, boundary_d), D, boundary_planes(gt_bits, H, W, boundary_d), G, T)
    return ious, da, bious


# --------------------------------------------------------------------------------------------------------------- data
class GroundTruth:
    """The parts of a YTVIS annotation document the evaluation reads (YTVOS.createIndex + YTVOSeval._prepare)"""

    def __init__(self, doc):
        if isinstance(doc, str):
            with open(doc) as fh:
                doc = json.load(fh)
        self.doc = doc
        self.videos = {v["id"]: v for v in doc.get("videos", [])}
        self.cat_ids = sorted(c["id"] for c in doc.get("categories", []))
        self.vid_ids = [int(v) for v in np.unique(list(self.videos.keys()))] if self.videos else []
        self.has_annotations = "annotations" in doc
        self.anns = defaultdict(list)                                  # video_id -> annotations in document order
        for a in doc.get("annotations", []):
            for s in a["segmentations"]:
                _frame_kind(s)                                         # polygons: refused up front
            self.anns[a["video_id"]].append(a)

    def video(self, vid):
        return self.videos[vid]

    def tracks(self, vid):
        """per ground truth of the video: id, category, crowd flag, ignore flag (= iscrowd, overwriting any `ignore` of the
        JSON), avg_area from the JSON's own `areas`"""
        out = []
        for a in self.anns.get(vid, []):
            crowd = a.get("iscrowd", 0)
            out.append(SimpleNamespace(id=a["id"], category_id=a["category_id"], iscrowd=int(crowd), ignore=bool("iscrowd" in a and crowd),
                                       avg_area=mean_area(a["areas"]), segmentations=a["segmentations"]))
        return out

    def decode(self, vid, device=None):
        """-> (bit planes [G*T, wpf] of the video's ground truth, G, T)"""
        v = self.videos[vid]
        gts = self.anns.get(vid, [])
        T = _common_length([a["segmentations"] for a in gts], vid)
        segs = [s for a in gts for s in a["segmentations"]]
        return decode_frames(segs, v["height"], v["width"], device), len(gts), T


def _common_length(tracks, vid, T=None):
    for t in tracks:
        if T is None:
            T = len(t)
        elif len(t) != T:
            raise ValueError(f"video {vid}: tracks of {len(t)} and {T} frames")
    return T if T is not None else 0


# --------------------------------------------------------------------------------------------------------------- host
class YTVISEval:
    """Matching, accumulation and summary of YTVOSeval (ytvoseval.py:267-510) on per-video IoU matrices.

    `evaluate(videos)` takes, per video id, {"dt_ids", "scores", "labels", "avg_areas", "ious"}: the detections in result order
    and their IoU against every ground truth of the video in document order ([D, G]).  Attributes after `evaluate`,
    `accumulate` and `summarize`: `ious[(video_id, category)]` (the reference's matrices, rows by descending score),
    `eval_vids` (the evaluateVid dicts, None where a video has neither), `eval["precision"]` [T,R,K,A,M], `eval["recall"]`
    [T,K,A,M], `stats` (12)."""

    def __init__(self, gt, use_cats=False, max_dets=(1, 10, 100)):
        self.gt = gt if isinstance(gt, GroundTruth) else GroundTruth(gt)
        self.params = SimpleNamespace(vidIds=list(self.gt.vid_ids), catIds=list(self.gt.cat_ids), iouThrs=IOU_THRS, recThrs=REC_THRS,
                                      maxDets=sorted(max_dets), areaRng=AREA_RNG, areaRngLbl=AREA_LBL, useCats=int(bool(use_cats)))
        self.ious, self.eval_vids, self.eval, self.stats = {}, [], {}, []

    def _group(self, items, cat):
        p = self.params
        if p.useCats:
            return [i for i, it in enumerate(items) if it == cat]
        return [i for c in p.catIds for i, it in enumerate(items) if it == c]

    def evaluate(self, videos):
        p = self.params
        for vid in videos:
            if vid not in self.gt.videos:
                raise ValueError(f"results for video {vid}, which the ground truth does not have")
        cats = p.catIds if p.useCats else [-1]
        self._gts, self._dts = {}, {}
        for vid in p.vidIds:
            gts = self.gt.tracks(vid)
            v = videos.get(vid)
            if v is None:
                v = {"dt_ids": [], "scores": [], "labels": [], "avg_areas": [], "ious": np.zeros((0, len(gts)))}
            ious = np.asarray(v["ious"], np.float64).reshape(len(v["scores"]), len(gts))
            gcat = [g.category_id for g in gts]
            for cat in cats:
                gi = self._group(gcat, cat)
                di = self._group(list(v["labels"]), cat)
                order = np.argsort([-v["scores"][i] for i in di], kind="mergesort")
                di = [di[i] for i in order][:p.maxDets[-1]]
                self._gts[vid, cat] = [gts[i] for i in gi]
                self._dts[vid, cat] = [SimpleNamespace(id=v["dt_ids"][i], score=v["scores"][i], avg_area=v["avg_areas"][i]) for i in di]
                if not gi and not di:
                    self.ious[vid, cat] = []
                else:
                    self.ious[vid, cat] = ious[np.ix_(np.asarray(di, np.intp), np.asarray(gi, np.intp))]
        self.eval_vids = [self._evaluate_video(vid, cat, rng, p.maxDets[-1]) for cat in cats for rng in p.areaRng for vid in p.vidIds]
        return self

    def _evaluate_video(self, vid, cat, rng, max_det):
        gt, dt = self._gts[vid, cat], self._dts[vid, cat]
        if not gt and not dt:
            return None
        g_ig = [1 if (g.ignore or g.avg_area < rng[0] or g.avg_area > rng[1]) else 0 for g in gt]
        gind = np.argsort(g_ig, kind="mergesort")
        gt = [gt[i] for i in gind]
        g_ig = np.array([g_ig[i] for i in gind])
        dt = dt[:max_det]                                                  # already in descending score order
        ious = self.ious[vid, cat]
        if len(ious) > 0:
            ious = ious[:, gind]
        T, G, D = len(IOU_THRS), len(gt), len(dt)
        gtm, dtm, dt_ig = np.zeros((T, G)), np.zeros((T, D)), np.zeros((T, D))
        crowd = [g.iscrowd for g in gt]
        if len(ious) != 0:
            for ti, t in enumerate(IOU_THRS):
                for di in range(D):
                    best, m = min(t, 1 - 1e-10), -1
                    for gi in range(G):
                        if gtm[ti, gi] > 0 and not crowd[gi]:
                            continue                                   # taken, and not a crowd
                        if m > -1 and g_ig[m] == 0 and g_ig[gi] == 1:
                            break                                      # matched a regular gt: ignored ones come last
                        if ious[di, gi] < best:
                            continue
                        best, m = ious[di, gi], gi
                    if m == -1:
                        continue
                    dt_ig[ti, di] = g_ig[m]
                    dtm[ti, di] = gt[m].id
                    gtm[ti, m] = dt[di].id
        out_of_rng = np.array([d.avg_area < rng[0] or d.avg_area > rng[1] for d in dt]).reshape((1, D))
        dt_ig = np.logical_or(dt_ig, np.logical_and(dtm == 0, np.repeat(out_of_rng, T, 0)))
        return {"video_id": vid, "category_id": cat, "aRng": rng, "maxDet": max_det, "dtIds": [d.id for d in dt], "gtIds": [g.id for g in gt],
                "dtMatches": dtm, "gtMatches": gtm, "dtScores": [d.score for d in dt], "gtIgnore": g_ig, "dtIgnore": dt_ig}

    def accumulate(self):
        p = self.params
        T, R, A, M = len(IOU_THRS), len(REC_THRS), len(AREA_RNG), len(p.maxDets)
        K = len(p.catIds) if p.useCats else 1
        I = len(p.vidIds)
        precision, recall, scores = -np.ones((T, R, K, A, M)), -np.ones((T, K, A, M)), -np.ones((T, R, K, A, M))
        for k, a, (m, max_det) in itertools.product(range(K), range(A), enumerate(p.maxDets)):
            E = [e for e in self.eval_vids[(k * A + a) * I:(k * A + a + 1) * I] if e is not None]
            if not E:
                continue
            dt_scores = np.concatenate([e["dtScores"][0:max_det] for e in E])
            inds = np.argsort(-dt_scores, kind="mergesort")
            dt_sorted = dt_scores[inds]
            dtm = np.concatenate([e["dtMatches"][:, 0:max_det] for e in E], axis=1)[:, inds]
            dt_ig = np.concatenate([e["dtIgnore"][:, 0:max_det] for e in E], axis=1)[:, inds]
            g_ig = np.concatenate([e["gtIgnore"] for e in E])
            npig = np.count_nonzero(g_ig == 0)
            if npig == 0:
                continue
            tp_sum = np.cumsum(np.logical_and(dtm, np.logical_not(dt_ig)), axis=1).astype(dtype=float)
            fp_sum = np.cumsum(np.logical_and(np.logical_not(dtm), np.logical_not(dt_ig)), axis=1).astype(dtype=float)
            for t in range(T):
                tp, fp = tp_sum[t], fp_sum[t]
                nd = len(tp)
                rc = tp / npig
                pr = tp / (fp + tp + np.spacing(1))
                recall[t, k, a, m] = rc[-1] if nd else 0
                pr = np.maximum.accumulate(pr[::-1])[::-1]             # precision envelope: max over the higher recalls
                ri = np.searchsorted(rc, REC_THRS, side="left")
                ok = ri < nd
                q, ss = np.zeros((R,)), np.zeros((R,))
                q[ok] = pr[ri[ok]]
                ss[ok] = dt_sorted[ri[ok]]
                precision[t, :, k, a, m] = q
                scores[t, :, k, a, m] = ss
        self.eval = {"params": p, "counts": [T, R, K, A, M], "precision": precision, "recall": recall, "scores": scores}
        return self

    def _summarize_one(self, ap, iou_thr=None, area="all", max_dets=100, out=print):
        p = self.params
        aind = [i for i, lbl in enumerate(AREA_LBL) if lbl == area]
        mind = [i for i, md in enumerate(p.maxDets) if md == max_dets]
        s = self.eval["precision" if ap else "recall"]
        if iou_thr is not None:
            s = s[np.where(iou_thr == IOU_THRS)[0]]
        s = s[:, :, :, aind, mind] if ap else s[:, :, aind, mind]
        mean_s = -1 if len(s[s > -1]) == 0 else np.mean(s[s > -1])
        iou = f"{IOU_THRS[0]:0.2f}:{IOU_THRS[-1]:0.2f}" if iou_thr is None else f"{iou_thr:0.2f}"
        title, kind = ("Average Precision", "(AP)") if ap else ("Average Recall", "(AR)")
        if out is not None:
            out(f" {title:<18} {kind} @[ IoU={iou:<9} | area={area:>6s} | maxDets={max_dets:>3d} ] = {mean_s:0.3f}")
        return mean_s

    def summarize(self, out=print):
        if not self.eval:
            raise RuntimeError("run accumulate() first")
        md = self.params.maxDets
        rows = [(1, None, "all", md[2]), (1, .5, "all", md[2]), (1, .75, "all", md[2]), (1, None, "small", md[2]), (1, None, "medium", md[2]),
                (1, None, "large", md[2]), (0, None, "all", md[0]), (0, None, "all", md[1]), (0, None, "all", md[2]), (0, None, "small", md[2]),
                (0, None, "medium", md[2]), (0, None, "large", md[2])]
        self.stats = np.zeros((12,))
        for i, r in enumerate(rows):
            self.stats[i] = self._summarize_one(*r, out=out)
        return self.stats


def derive_results(stats):
    """YTVISEvaluator._derive_coco_results: the 9 named metrics x 100, nan where the stat is -1"""
    return {m: float(stats[i] * 100 if stats[i] >= 0 else "nan") for i, m in enumerate(METRICS) if i < len(stats)}


def _video_record(gt, vid, dt_bits, D, T, H, W, device, dilation_ratio=None):
    """IoU of D detection tracks (bit planes [D*T, wpf]) against the video's ground truth; -> (ious [D, G], frame areas [D, T]),
    and with a dilation_ratio (Boundary AP) the boundary IoUs [D, G] as a third item: the video is decoded once for both"""
    v = gt.video(vid)
    if (v["height"], v["width"]) != (H, W):
        raise ValueError(f"video {vid} is {v['height']}x{v['width']}, its predictions {H}x{W}")
    gt_bits, G, Tg = gt.decode(vid, device)
    if G and D and Tg != T:
        raise ValueError(f"video {vid}: predictions of {T} frames, ground truth of {Tg}")
    if D == 0:
        rec = np.zeros((0, G)), np.zeros((0, T), np.int64)
    elif G == 0:
        rec = np.zeros((D, 0)), plane_areas(dt_bits).cpu().numpy().astype(np.int64).reshape(D, T)
    elif dilation_ratio is None:
        return video_ious(dt_bits, D, gt_bits, G, T)
    else:
        return video_ious(dt_bits, D, gt_bits, G, T, boundary_d=boundary_dilation(H, W, dilation_ratio), size=(H, W))
    return rec if dilation_ratio is None else rec + (np.zeros((D, G)),)


def evaluate_ytvis(gt, results, *, use_cats=False, max_dets=(1, 10, 100), device=None, iou_type="segm", dilation_ratio=0.02):
    """Score an existing results list / results.json (what YTVISEvaluator writes, the reference's included) against a YTVIS
    annotation document / file, as _evaluate_predictions_on_coco does (useCats = 0 by default).  Returns the YTVISEval after
    evaluate + accumulate (call .summarize() for the table and .stats).  Detection ids are result positions + 1 (loadRes).
    iou_type="boundary": Boundary AP -- matching on min(mask IoU, boundary IoU) at dilation_ratio, all else as for "segm"."""
    if iou_type not in ("segm", "boundary"):
        raise ValueError(f"iou_type {iou_type!r}: 'segm' or 'boundary'")
    ratio = dilation_ratio if iou_type == "boundary" else None
    if isinstance(results, str):
        with open(results) as fh:
            results = json.load(fh)
    gt = gt if isinstance(gt, GroundTruth) else GroundTruth(gt)
    by_vid = defaultdict(list)
    for n, r in enumerate(results):
        if r["video_id"] not in gt.videos:
            raise ValueError(f"results for video {r['video_id']}, which the ground truth does not have")
        by_vid[r["video_id"]].append(n)
    videos = {}
    for vid, idx in by_vid.items():
        v = gt.video(vid)
        H, W = v["height"], v["width"]
        tracks = [results[n]["segmentations"] for n in idx]
        T = _common_length(tracks, vid)
        bits = decode_frames([s for t in tracks for s in t], H, W, device)
        ious, fa, *bious = _video_record(gt, vid, bits, len(idx), T, H, W, device, ratio)
        if bious:
            ious = np.minimum(ious, bious[0])
        areas = [[int(fa[d, t]) if tracks[d][t] else None for t in range(T)] for d in range(len(idx))]   # loadRes areas
        videos[vid] = {"dt_ids": [n + 1 for n in idx], "scores": [results[n]["score"] for n in idx],
                       "labels": [results[n]["category_id"] for n in idx], "avg_areas": [mean_area(a) for a in areas], "ious": ious}
    return YTVISEval(gt, use_cats, max_dets).evaluate(videos).accumulate()


class YTVISEvaluator:
    """Drop-in for the reference's YTVISEvaluator (data_video/ytvis_eval.py), `YTVISEvaluator(dataset_name, cfg, True, output_dir)`
    as train_net_video.py:87 builds it.  `dataset_name` resolves to MetadataCatalog.get(name).json_file when detectron2 is
    importable; otherwise pass `json_file=` (a path or a loaded document).  `process` scores one video on the device at once
    and keeps only its IoU matrix and detection scores / categories / areas (plus its RLE when `output_dir` is set, for the
    results.json that evaluate() writes).  boundary=True: Boundary AP as well -- `process` keeps the video's boundary IoU matrix
    beside the mask one (one decode for both), evaluate() returns {"segm", "boundary"} and keeps `ytvis_eval_boundary`."""

    def __init__(self, dataset_name=None, tasks=None, distributed=True, output_dir=None, *, json_file=None, dataset_id_to_contiguous_id=None,
                 boundary=False, dilation_ratio=0.02):
        self._distributed, self._output_dir, self._tasks = distributed, output_dir, tasks
        self._dilation_ratio = dilation_ratio if boundary else None
        if json_file is None:
            if dataset_name is None:
                raise ValueError("YTVISEvaluator needs a dataset_name (with detectron2) or json_file=")
            try:
                from detectron2.data import MetadataCatalog
            except ImportError as e:
                raise ValueError("detectron2 is not importable: pass json_file= (a path or a loaded document)") from e
            meta = MetadataCatalog.get(dataset_name)
            json_file = meta.json_file
            if dataset_id_to_contiguous_id is None:
                dataset_id_to_contiguous_id = getattr(meta, "thing_dataset_id_to_contiguous_id", None)
        self._gt = GroundTruth(json_file)
        self._do_evaluation = self._gt.has_annotations
        self._reverse = None
        if dataset_id_to_contiguous_id:
            ids = list(dataset_id_to_contiguous_id.values())
            assert min(ids) == 0 and max(ids) == len(ids) - 1
            self._reverse = {v: k for k, v in dataset_id_to_contiguous_id.items()}
        self.reset()

    def reset(self):
        self._records = []

    def process(self, inputs, outputs):
        """inputs: one video ({"video_id", ...}); outputs: what inference_video returns -- pred_masks as CPU bool tensors
        [T,H,W] per prediction, as RLE lists (rle=True), or as a CUDA bool/u8 tensor [K,T,H,W] / list of CUDA tensors."""
        import torch
        from . import ops
        assert len(inputs) == 1, "More than one inputs are loaded for inference!"
        vid = inputs[0]["video_id"]
        scores = [float(s) for s in outputs["pred_scores"]]
        labels = [int(l) for l in outputs["pred_labels"]]
        if self._reverse is not None:
            for l in labels:
                assert l < len(self._reverse), f"A prediction has class={l}, but the dataset only has {len(self._reverse)} classes"
            labels = [self._reverse[l] for l in labels]
        masks = outputs["pred_masks"]
        D = len(scores)
        dev = torch.device("cuda", torch.cuda.current_device())
        rles = None
        if D and (outputs.get("pred_masks_format") == "coco_rle" or isinstance(masks[0], (list, tuple))):
            T = _common_length(masks, vid)
            segs = [s for m in masks for s in m]
            first = next((s for s in segs if s), None)
            if vid in self._gt.videos:
                H, W = self._gt.video(vid)["height"], self._gt.video(vid)["width"]
            else:
                H, W = (int(v) for v in first["size"])
            bits = decode_frames(segs, H, W, dev)
            present = [[bool(s) for s in m] for m in masks]
            if self._output_dir:
                rles = [[dict(s, counts=s["counts"].decode() if isinstance(s["counts"], bytes) else s["counts"]) if s else s for s in m]
                        for m in masks]
        elif D:
            if isinstance(masks, torch.Tensor):
                md = masks
            elif masks[0].is_cuda:
                md = torch.stack(list(masks))
            else:
                host = torch.stack([torch.as_tensor(m) for m in masks])
                if host.dtype == torch.bool:
                    host = host.view(torch.uint8)
                md = host.pin_memory().to(dev, non_blocking=True)
            if md.dtype == torch.bool:
                md = md.view(torch.uint8)
            md = md.to(dev).contiguous()
            _, T, H, W = md.shape
            bits = ops.pack_mask_bits(md.view(D * T, H * W))
            present = [[True] * T for _ in range(D)]
            if self._output_dir:
                from .rle import encode_video_predictions
                rles = encode_video_predictions(md)
        else:
            T = H = W = 0
            bits, present = None, []
        rec = {"video_id": vid, "scores": scores, "labels": labels, "rles": rles}
        if self._do_evaluation:
            if vid not in self._gt.videos:
                raise ValueError(f"video {vid} is not in the ground truth")
            if D:
                ious, fa, *bious = _video_record(self._gt, vid, bits, D, T, H, W, dev, self._dilation_ratio)
            else:
                ious, fa = np.zeros((0, len(self._gt.anns.get(vid, [])))), np.zeros((0, 0), np.int64)
                bious = [ious] if self._dilation_ratio is not None else []
            rec["ious"] = ious
            if bious:
                rec["boundary_ious"] = bious[0]
            rec["avg_areas"] = [mean_area([int(fa[d, t]) if present[d][t] else None for t in range(fa.shape[1])]) for d in range(D)]
        self._records.append(rec)

    def _gather(self):
        import torch.distributed as dist
        if self._distributed and dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            parts = [None] * dist.get_world_size()
            dist.all_gather_object(parts, self._records)
            if dist.get_rank() != 0:
                return None
            return list(itertools.chain(*parts))
        return self._records

    def evaluate(self):
        records = self._gather()
        if records is None:
            return {}
        if sum(len(r["scores"]) for r in records) == 0:
            _log.warning("[YTVISEvaluator] Did not receive valid predictions.")
            return {}
        if self._output_dir:
            os.makedirs(self._output_dir, exist_ok=True)
            preds = [{"video_id": r["video_id"], "score": s, "category_id": l, "segmentations": m}
                     for r in records for s, l, m in zip(r["scores"], r["labels"], r["rles"])]
            with open(os.path.join(self._output_dir, "results.json"), "w") as fh:
                fh.write(json.dumps(preds))
        results = OrderedDict()
        if not self._do_evaluation:
            _log.info("Annotations are not available for evaluation.")
            return results
        videos, nid = {}, 0
        for r in records:                                   # detection ids: positions in the gathered prediction list + 1
            D = len(r["scores"])
            v = videos.setdefault(r["video_id"], {"dt_ids": [], "scores": [], "labels": [], "avg_areas": [], "ious": [], "boundary_ious": []})
            v["dt_ids"] += list(range(nid + 1, nid + D + 1))
            v["scores"] += r["scores"]; v["labels"] += r["labels"]; v["avg_areas"] += r["avg_areas"]
            v["ious"].append(r["ious"])
            if self._dilation_ratio is not None:
                v["boundary_ious"].append(r["boundary_ious"])
            nid += D
        for v in videos.values():
            v["ious"] = np.concatenate(v["ious"], 0)
        ev = YTVISEval(self._gt, use_cats=False, max_dets=(1, 10, 100)).evaluate(videos).accumulate()
        ev.summarize()
        self.ytvis_eval = ev
        results["segm"] = derive_results(ev.stats)
        if self._dilation_ratio is not None:                # Boundary AP: the same detections matched on min(mask, boundary) IoU
            bvideos = {vid: dict(v, ious=np.minimum(v["ious"], np.concatenate(v["boundary_ious"], 0))) for vid, v in videos.items()}
            evb = YTVISEval(self._gt, use_cats=False, max_dets=(1, 10, 100)).evaluate(bvideos).accumulate()
            evb.summarize()
            self.ytvis_eval_boundary = evb
            results["boundary"] = derive_results(evb.stats)
        return results


def main(argv=None):
    ap = argparse.ArgumentParser(description="YTVIS video-instance mask AP / AR of a results.json")
    ap.add_argument("--gt", required=True, help="YTVIS annotation JSON")
    ap.add_argument("--results", required=True, help="results.json (list of {video_id, score, category_id, segmentations})")
    ap.add_argument("--use-cats", action="store_true", help="per-category matching (the stock YTVIS protocol); default pools categories")
    ap.add_argument("--iou-type", choices=("segm", "boundary"), default="segm", help="boundary: Boundary AP, matching on min(mask IoU, boundary IoU)")
    ap.add_argument("--dilation-ratio", type=float, default=0.02, help="boundary band width as a fraction of the image diagonal (--iou-type boundary)")
    a = ap.parse_args(argv)
    evaluate_ytvis(a.gt, a.results, use_cats=a.use_cats, iou_type=a.iou_type, dilation_ratio=a.dilation_ratio).summarize()


if __name__ == "__main__":
    main()
