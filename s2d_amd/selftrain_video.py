"""Video self-training rounds: the previous round's YTVIS annotation file + this round's results.json -> the next round's file.

    python -m s2d_amd.selftrain_video --results-file results.json --prev-ann round0.json --save-path round1.json \\
        [--gt-annotation-file gt.json] [--score-threshold 0.75] [--frames annotated|all]

The step that closes the video loop with a MERGE (train -> evaluate -> selftrain_video -> train --train-json round1.json), as
s2d_amd.selftrain closes the image loop.  keymask.results_to_annotations (the reference's keymask_ident/
convert_results_to_annotations.py) only thresholds results.json: an object that discovery found as a keymask track but the student
does not yet score above the threshold is gone from the next round for good.  Here the confident predictions are kept and the
previous round's tracks that no kept prediction covers are added.  THE MERGE RULE IS THIS PROJECT'S OWN: the image rule of
get_self_training_ann.py (s2d_amd.selftrain) carried to tubes.  The reference has no video merge.

  * a prediction is kept when score >= threshold, in file order, grouped by video_id; a prediction of a video absent from `videos`
    is skipped, as the converter does;
  * tube counts of a previous track p and a kept prediction q of the same video over a frame set F:
        inter = sum_{t in F} |p_t & q_t|        union = sum_{t in F} (|p_t| + |q_t| - |p_t & q_t|)
    with a None segmentation an empty plane;
  * --frames all: F is every frame, the YTVIS evaluator's rule (ytvis_eval.video_ious computes the same integers);
    --frames annotated (the default): F is the frames where p HAS a segmentation.  A keymask track annotates a handful of frames.
    Against a dense 36-frame prediction of the same object its all-frame IoU is roughly (key frames / all frames), far below one
    half, so under `all` nearly every keymask would survive beside the prediction that duplicates it.  On its own frames the pair
    is compared like two image masks;
  * p is kept iff EVERY kept q of its video has 2 * inter < union, decided in int64 (the image merge's integer rule; the threshold
    stays 0.5 and there is no float anywhere).  A video without kept predictions keeps all its tracks.  union == 0 -- a track
    with no annotated frame, or empty masks on both sides -- fails the test and the track is dropped, as in
    s2d_selftrain_keep_ragged;
  * output order: the videos with previous annotations, in order of first appearance among them, each with its kept predictions in
    file order and then its surviving previous tracks in their own order; then the videos that have only predictions, in order of
    first appearance.  `id` runs 1.. in that order;
  * a prediction becomes an annotation exactly as results_to_annotations.convert writes it (bboxes float [x, y, w, h] or None,
    areas int or None, iscrowd 0, height, width, length, category_id) and keeps its `score`; surviving previous tracks are copied
    unchanged but for `id`;
  * `videos`, `info`, `licenses` come from --gt-annotation-file when given, else from the previous file; `categories` from the
    previous file.

Where this differs from convert_results_to_annotations.py, on purpose:
  * the previous round's annotations are merged in, not thrown away (above);
  * `id` is the position in the output, 1.., not the prediction's index in results.json + 1 (skipped predictions use up no ids:
    the ids of the two sources would collide otherwise);
  * `score` is kept on a prediction's annotation;
  * --gt-annotation-file is optional: the previous file has `videos` too; `info` / `licenses` the source lacks are left out;
  * an RLE whose `size` is not the video's [height, width] is a ValueError naming the video (the reference decodes it as it is),
    and so is a previous annotation of a video absent from `videos` or with a frame count that is not the video's `length`;
  * a merged annotation whose category_id is not among the output categories is refused, naming the video: the next round's
    load_ytvis_train would fail on it far from the cause;
  * the inputs are not modified: output annotations are copies.

Device side, per chunk of videos of different sizes and lengths (bounded by CHUNK_WORDS / CHUNK_VIDEOS) SIX library calls however
many videos the chunk holds: the ragged RLE parse, decode and tight boxes (rle_ragged.decode_ragged; a track is its T frame planes
back to back, an absent frame a plane with 0 runs), the plane areas (s2d_mask_plane_areas_ragged_u32), the tube counts
(s2d_tube_counts_ragged) and the keep rule (s2d_selftrain_keep_tube_ragged), then ONE read-back of the keep flags, areas and boxes.
Only videos with a kept prediction enter a chunk; their previous tracks ride along.  A video whose planes exceed CHUNK_WORDS is
alone in its chunk and goes through in slabs of frames: five calls per slab, the tube counts accumulating, one keep call and still
one read-back.  RLE decode is restated from pycocotools (absent from the project's machines): parity unpinned."""
import argparse
import json
import time
from collections import Counter
from types import SimpleNamespace

import numpy as np

from . import coco_eval

CHUNK_VIDEOS = 1024
LIB_CALLS = Counter()          # this module's library calls by export name, "chunks", "slabs" and "readbacks"; the decode calls are
#                                rle_ragged.LIB_CALLS
FRAME_SETS = ("annotated", "all")
VID_COLS = 11


def _chunk_words():
    return coco_eval.CHUNK_WORDS               # read at call time: one bound for every ragged path


def tube_keep_rule(inter, union):
    """the integer keep rule on numpy arrays: inter, union [D, G] -> bool [D], True where every g has 2 * inter < union (all True
    for G == 0)"""
    i, u = np.asarray(inter, np.int64), np.asarray(union, np.int64)
    return (2 * i < u).all(axis=1)


# ------------------------------------------------------------------------------------------------------------------ device
def _slab_tables(part, t0s, t1s, staged, frames):
    """the host tables of one slab: videos int64 [N, 11], tiles int32 [n, 3], present u8, max T * wpp"""
    vids = np.zeros((len(part), VID_COLS), np.int64)
    tiles, present = [], []
    d0 = g0 = pair0 = pres0 = 0
    max_tw = 0
    for n, (it, t0, t1) in enumerate(zip(part, t0s, t1s)):
        D, G, T = len(it.dsegs), len(it.gsegs), t1 - t0
        wpp = (it.H * it.W + 31) // 32
        p_word = int(staged.plane[int(staged.plane0[n]), 0]) if (D + G) * T else 0
        vids[n] = p_word, p_word + D * T * wpp, wpp, it.H * it.W, T, D, G, d0, g0, pair0, pres0
        if D and G:
            ntd, ntg = (D + 7) // 8, (G + 7) // 8
            tiles.append(np.stack([np.full(ntd * ntg, n), np.repeat(np.arange(ntd), ntg), np.tile(np.arange(ntg), ntd)], 1))
            max_tw = max(max_tw, T * wpp)
        for segs in it.dsegs:
            present.append(np.ones(T, np.uint8) if frames == "all" else np.array([s is not None for s in segs[t0:t1]], np.uint8))
        d0, g0, pair0, pres0 = d0 + D, g0 + G, pair0 + D * G, pres0 + D * T
    tiles_h = np.concatenate(tiles).astype(np.int32) if tiles else np.zeros((0, 3), np.int32)
    pres_h = np.concatenate(present).astype(np.uint8) if present else np.zeros(0, np.uint8)
    return vids, tiles_h, pres_h, max_tw


def device_merge(chunk, frames="annotated", device=None, seconds=None, counts=None):
    """the device side of one chunk (SimpleNamespace(items: work items of plan_round with dsegs / gsegs filled, slabs: None or the
    [(t0, t1)] frame ranges of its single video)) -> (keep int32 [sum D], areas int64 [Q planes], boxes int32 [Q planes, 4]) as numpy
    arrays, Q planes = the kept predictions' frames, video after video, prediction after prediction.  seconds: a dict that collects
    device-inclusive phase times; counts: a dict that receives the raw `inter` / `union` int64 arrays (one more read-back: tests)"""
    import torch
    from . import ops
    from ._lib import lib
    from .rle_ragged import _upload, decode_ragged, stage_rle_ragged
    dev = coco_eval._device(device)
    part = chunk.items

    def tick(name, t0):
        if seconds is not None:
            torch.cuda.synchronize(dev)
            seconds[name] = seconds.get(name, 0.0) + time.perf_counter() - t0
        return time.perf_counter()

    def call(name, *args):
        LIB_CALLS[name] += 1
        lib().call(name, *args)

    slabs = chunk.slabs if chunk.slabs else [None]
    nd = sum(len(it.dsegs) for it in part)
    n_pairs = sum(len(it.dsegs) * len(it.gsegs) for it in part)
    ranges = [[(0, it.T) for it in part] if s is None else [s] for s in slabs]
    n_planes = [sum((len(it.dsegs) + len(it.gsegs)) * (t1 - t0) for it, (t0, t1) in zip(part, r)) for r in ranges]
    out = torch.empty((5 * sum(n_planes) + nd,), device=dev, dtype=torch.int32)       # per slab boxes, areas; then the keep flags
    inter = torch.empty((max(n_pairs, 1),), device=dev, dtype=torch.int64)
    union = torch.empty((max(n_pairs, 1),), device=dev, dtype=torch.int64)
    st = ops._stream()
    off, vids_d = 0, None
    for k, (r, P) in enumerate(zip(ranges, n_planes)):
        t0 = time.perf_counter()
        LIB_CALLS["slabs"] += 1
        t0s, t1s = [a for a, _ in r], [b for _, b in r]
        segs = [[s for tr in it.dsegs + it.gsegs for s in tr[a:b]] for it, a, b in zip(part, t0s, t1s)]
        staged = stage_rle_ragged(segs, [(it.H, it.W) for it in part], names=[f"video {it.vid}" for it in part])
        vids, tiles_h, pres_h, max_tw = _slab_tables(part, t0s, t1s, staged, frames)
        if staged.P != P or int(pres_h.size) != sum(len(it.dsegs) * (b - a) for it, a, b in zip(part, t0s, t1s)):
            raise RuntimeError(f"slab tables of {staged.P} planes for {P}")
        t0 = tick("stage", t0)
        dec = decode_ragged(staged, dev, bbox_out=out[off:off + 4 * P].view(P, 4))
        if P:
            call("s2d_mask_plane_areas_ragged_u32", dec.bits, dec.plane_dev, P, staged.words, out[off + 4 * P:off + 5 * P], st)
        t0 = tick("decode", t0)
        vids_d, tiles_d, pres_d = _upload([vids, tiles_h, pres_h], dev)
        if n_pairs:
            call("s2d_tube_counts_ragged", dec.bits, staged.words, vids_d, len(part), pres_d, int(pres_h.size),
                 tiles_d if len(tiles_h) else None, len(tiles_h), max_tw, inter, union, n_pairs, 1 if k else 0, st)
        t0 = tick("counts", t0)
        off += 5 * P
    t0 = time.perf_counter()
    if nd:
        call("s2d_selftrain_keep_tube_ragged", inter if n_pairs else None, union if n_pairs else None, n_pairs, vids_d, len(part),
             out[off:], nd, st)
    LIB_CALLS["readbacks"] += 1
    host = out.cpu().numpy()
    tick("keep", t0)
    if counts is not None:
        counts["inter"], counts["union"] = inter[:n_pairs].cpu().numpy(), union[:n_pairs].cpu().numpy()
    areas, boxes = [], []
    off = 0
    for r, P in zip(ranges, n_planes):
        bx, ar = host[off:off + 4 * P].reshape(P, 4), host[off + 4 * P:off + 5 * P].view(np.uint32).astype(np.int64)
        p0, sa, sb = 0, [], []
        for it, (a, b) in zip(part, r):
            D, G, T = len(it.dsegs), len(it.gsegs), b - a
            sa.append(ar[p0 + D * T:p0 + (D + G) * T].reshape(G, T))
            sb.append(bx[p0 + D * T:p0 + (D + G) * T].reshape(G, T, 4))
            p0 += (D + G) * T
        areas.append(sa)
        boxes.append(sb)
        off += 5 * P
    if chunk.slabs:                                                               # one video: its slabs side by side along T
        areas, boxes = [[np.concatenate([s[0] for s in areas], 1)]], [[np.concatenate([s[0] for s in boxes], 1)]]
    flat_a = np.concatenate([a.reshape(-1) for a in areas[0]]) if part else np.zeros(0, np.int64)
    flat_b = np.concatenate([b.reshape(-1, 4) for b in boxes[0]]) if part else np.zeros((0, 4), np.int32)
    return host[off:].copy(), flat_a, flat_b


# ------------------------------------------------------------------------------------------------------------------ host
def _check_track(e, v, what):
    vid, T, size = v["id"], v["length"], [v["height"], v["width"]]
    segs = e.get("segmentations")
    if not isinstance(segs, (list, tuple)) or len(segs) != T:
        n = len(segs) if isinstance(segs, (list, tuple)) else None
        raise ValueError(f"Number of frames in video {vid} ({T}) does not match the number of segmentations ({n}) of {what}")
    for s in segs:
        if s is None:
            continue
        if not isinstance(s, dict) or "counts" not in s:
            raise ValueError(f"video {vid}: {what} with a segmentation that is not an RLE (polygons are not supported: convert them)")
        if [int(x) for x in s.get("size", [])] != size:
            raise ValueError(f"video {vid}: {what} with an RLE of size {s.get('size')} in a video of size {size}")
    return list(segs)


def plan_round(prev_doc, results, videos_doc=None, threshold=0.75):
    """-> the per-video work items in output order (videos with previous annotations, then videos with predictions only), each a
    SimpleNamespace(vid, H, W, T, prev, pred: the entries; dsegs, gsegs: per track its T segmentations, dsegs empty where the
    device does not need them; keep, areas [G, T], boxes [G, T, 4]: filled by merge_round)"""
    videos = {v["id"]: v for v in (videos_doc if videos_doc is not None else prev_doc)["videos"]}
    pred, prev = {}, {}
    for p in results:
        if p["score"] >= threshold and p["video_id"] in videos:
            pred.setdefault(p["video_id"], []).append(p)
    for a in prev_doc["annotations"]:
        if a["video_id"] not in videos:
            raise ValueError(f"video {a['video_id']}: an annotation for a video that `videos` does not have")
        prev.setdefault(a["video_id"], []).append(a)
    items = []
    for vid in list(prev) + [k for k in pred if k not in prev]:
        v = videos[vid]
        a, p = prev.get(vid, []), pred.get(vid, [])
        dsegs = [_check_track(e, v, "a previous annotation") for e in a]
        gsegs = [_check_track(e, v, "a prediction") for e in p]
        items.append(SimpleNamespace(vid=vid, H=int(v["height"]), W=int(v["width"]), T=int(v["length"]), video=v, prev=a, pred=p,
                                     dsegs=dsegs if p else [], gsegs=gsegs, keep=[True] * len(a), areas=None, boxes=None))
    return items


def _chunks(items):
    """the items with a kept prediction, cut at CHUNK_WORDS / CHUNK_VIDEOS; a video over the bound is alone, in slabs of frames"""
    limit = _chunk_words()
    chunk, words = [], 0
    for it in items:
        if not it.gsegs:
            continue
        per_frame = (len(it.dsegs) + len(it.gsegs)) * ((it.H * it.W + 31) // 32)
        w = per_frame * it.T
        if w > limit:
            if chunk:
                yield SimpleNamespace(items=chunk, slabs=None)
                chunk, words = [], 0
            step = max(1, limit // per_frame)
            yield SimpleNamespace(items=[it], slabs=[(t, min(t + step, it.T)) for t in range(0, it.T, step)])
            continue
        if chunk and (words + w > limit or len(chunk) >= CHUNK_VIDEOS):
            yield SimpleNamespace(items=chunk, slabs=None)
            chunk, words = [], 0
        chunk.append(it)
        words += w
    if chunk:
        yield SimpleNamespace(items=chunk, slabs=None)


def merge_round(prev_doc, results, videos_doc=None, threshold=0.75, frames="annotated", device=None, device_fn=None, seconds=None):
    """loaded documents -> the next round's annotation document (module docstring).  videos_doc: the document `videos`, `info` and
    `licenses` come from (default: prev_doc).  device_fn: (chunk, frames) -> (keep [sum D], areas [Q planes], boxes [Q planes, 4])
    replaces the device side (device_merge), so the host logic runs without a device; seconds: a dict that collects the phase
    times (stage, decode, counts, keep: device-inclusive; assemble)."""
    if frames not in FRAME_SETS:
        raise ValueError(f"frames must be one of {FRAME_SETS}, not {frames!r}")
    if device_fn is None:
        device_fn = lambda chunk, fr: device_merge(chunk, fr, device, seconds)     # noqa: E731
    src = videos_doc if videos_doc is not None else prev_doc
    t0 = time.perf_counter()
    items = plan_round(prev_doc, results, videos_doc, threshold)
    host = time.perf_counter() - t0
    for chunk in _chunks(items):
        LIB_CALLS["chunks"] += 1
        keep, areas, boxes = device_fn(chunk, frames)
        t0 = time.perf_counter()
        keep, areas, boxes = np.asarray(keep).reshape(-1), np.asarray(areas).reshape(-1), np.asarray(boxes).reshape(-1, 4)
        nd, nq = sum(len(it.dsegs) for it in chunk.items), sum(len(it.gsegs) * it.T for it in chunk.items)
        if len(keep) != nd or len(areas) != nq or len(boxes) != nq:
            raise ValueError(f"device_fn returned {len(keep)} flags, {len(areas)} areas and {len(boxes)} boxes for {nd} tracks and {nq} planes")
        d0 = q0 = 0
        for it in chunk.items:
            D, G, T = len(it.dsegs), len(it.gsegs), it.T
            if D:
                it.keep = [bool(k) for k in keep[d0:d0 + D]]
            it.areas, it.boxes = areas[q0:q0 + G * T].reshape(G, T).tolist(), boxes[q0:q0 + G * T].reshape(G, T, 4).tolist()
            d0, q0 = d0 + D, q0 + G * T
        host += time.perf_counter() - t0
    t0 = time.perf_counter()
    out = {k: src[k] for k in ("info", "licenses") if k in src}
    out["videos"] = src["videos"]
    out["categories"] = prev_doc["categories"]
    cats = {c["id"] for c in out["categories"]}
    merged = []

    def emit(it, a):
        if a.get("category_id") not in cats:
            raise ValueError(f"video {it.vid}: category_id {a.get('category_id')!r} is not among the output categories {sorted(cats)}")
        a["id"] = len(merged) + 1
        merged.append(a)

    for it in items:
        for g, p in enumerate(it.pred):
            segs = it.gsegs[g]
            emit(it, {"video_id": it.vid, "iscrowd": 0, "height": it.video["height"], "width": it.video["width"], "length": it.video["length"],
                      "segmentations": segs,
                      "bboxes": [[float(x) for x in it.boxes[g][t]] if s is not None else None for t, s in enumerate(segs)],
                      "areas": [int(it.areas[g][t]) if s is not None else None for t, s in enumerate(segs)],
                      "category_id": p["category_id"], "id": None, "score": p["score"]})
        for k, a in enumerate(it.prev):
            if it.keep[k]:
                emit(it, dict(a))
    out["annotations"] = merged
    if seconds is not None:
        seconds["assemble"] = seconds.get("assemble", 0.0) + host + time.perf_counter() - t0
    return out


def merge_files(results_file, prev_ann, save_path, gt_annotation_file=None, threshold=0.75, frames="annotated", device=None,
                device_fn=None, seconds=None, cleanup=None):
    """the command line on paths -> the written document.  cleanup: a clean_annotations.cleanup_options dict; when it asks for
    anything the merged document's masks are cleaned just before it is written (the merge sees the masks as they came)"""
    t0 = time.perf_counter()
    with open(results_file) as fh:
        results = json.load(fh)
    with open(prev_ann) as fh:
        prev_doc = json.load(fh)
    gt = None
    if gt_annotation_file:
        with open(gt_annotation_file) as fh:
            gt = json.load(fh)
    t_json = time.perf_counter() - t0
    doc = merge_round(prev_doc, results, gt, threshold, frames, device=device, device_fn=device_fn, seconds=seconds)
    if cleanup:
        from .clean_annotations import clean_merged
        doc = clean_merged(doc, cleanup, device=device)
    t0 = time.perf_counter()
    with open(save_path, "w") as fh:
        json.dump(doc, fh)
    if seconds is not None:
        seconds["json"] = seconds.get("json", 0.0) + t_json + time.perf_counter() - t0
    return doc


def main(argv=None):
    ap = argparse.ArgumentParser(description="Merge a results.json into the previous round's YTVIS annotation file.")
    ap.add_argument("--results-file", required=True, help="this round's predictions (results.json)")
    ap.add_argument("--prev-ann", required=True, help="the previous round's annotation JSON (tracks, categories)")
    ap.add_argument("--save-path", required=True, help="where the next round's annotation JSON is written")
    ap.add_argument("--gt-annotation-file", default=None, help="take info, licenses and videos from this file instead of --prev-ann")
    ap.add_argument("--score-threshold", type=float, default=0.75)
    ap.add_argument("--frames", choices=FRAME_SETS, default="annotated",
                    help="frames a previous track is compared on: those it annotates (default), or all (the YTVIS evaluator's IoU)")
    from .clean_annotations import add_cleanup_arguments, cleanup_options
    a = add_cleanup_arguments(ap).parse_args(argv)
    doc = merge_files(a.results_file, a.prev_ann, a.save_path, a.gt_annotation_file, a.score_threshold, a.frames, cleanup=cleanup_options(a))
    print("Done: {} videos; {} anns.".format(len(doc["videos"]), len(doc["annotations"])))


if __name__ == "__main__":
    main()
