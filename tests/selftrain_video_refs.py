"""Helpers of the video self-training merge tests: a pure numpy / Python restatement of s2d_amd.selftrain_video written from its
behaviour list (RLE decode by the oracle's decoder, tube counts as Python integers on dense masks, the merge as plain loops), a
numpy device_fn for merge_round, and the case builders the CPU and the GPU tests share."""
from types import SimpleNamespace

import numpy as np

from tests import selftrain_refs as R

# the kernel chunk's video sizes: 1 x 1; 35 pixels (a 3-bit tail in the second word); 1023 (a 31-bit tail); 4096 (no tail, rows
# word-aligned); 4000 (no tail, rows not word-aligned)
KERNEL_SIZES = [(1, 1), (5, 7), (31, 33), (64, 64), (40, 100)]


# ------------------------------------------------------------------------------------------------------------------ counts
def track_masks(segs, H, W):
    """a track's segmentations -> bool [T, H, W]; None -> an empty plane"""
    return np.stack([R.seg_mask(s, H, W) for s in segs]) if len(segs) else np.zeros((0, H, W), bool)


def tube_counts(p_segs, q_segs, H, W, frames):
    """-> (inter, union) of one pair as Python integers over the frame set"""
    inter = union = 0
    for sp, sq in zip(p_segs, q_segs):
        if frames == "annotated" and sp is None:
            continue
        a, b = R.seg_mask(sp, H, W), R.seg_mask(sq, H, W)
        i = int((a & b).sum())
        inter += i
        union += int(a.sum()) + int(b.sum()) - i
    return inter, union


def keep_track(p_segs, q_tracks, H, W, frames):
    for q in q_tracks:
        i, u = tube_counts(p_segs, q, H, W, frames)
        if not 2 * i < u:
            return False
    return True


def chunk_counts(items, frames):
    """the rows s2d_tube_counts_ragged writes for a chunk: (inter, union) lists of Python integers, video after video, [D][G] each"""
    inter, union = [], []
    for it in items:
        for p in it.dsegs:
            for q in it.gsegs:
                i, u = tube_counts(p, q, it.H, it.W, frames)
                inter.append(i)
                union.append(u)
    return inter, union


def numpy_device(chunk, frames):
    """merge_round's device_fn on the host: (keep [sum D], areas [Q planes], boxes [Q planes, 4])"""
    keep, areas, boxes = [], [], []
    for it in chunk.items:
        keep += [keep_track(p, it.gsegs, it.H, it.W, frames) for p in it.dsegs]
        for q in it.gsegs:
            for m in track_masks(q, it.H, it.W):
                areas.append(int(m.sum()))
                boxes.append(R.box_of(m))
    return np.array(keep, np.int32), np.array(areas, np.int64), np.array(boxes, np.int32).reshape(-1, 4)


def numpy_bbox_area(segs, H, W):
    """results_to_annotations.convert's bbox_area_fn on the host"""
    masks = [None if s is None else R.seg_mask(s, H, W) for s in segs]
    return ([None if m is None else [float(v) for v in R.box_of(m)] for m in masks], [None if m is None else int(m.sum()) for m in masks])


# ------------------------------------------------------------------------------------------------------------------ the tool
def reference_merge(prev_doc, results, videos_doc=None, threshold=0.75, frames="annotated"):
    """the tool restated on dense masks, video by video"""
    src = prev_doc if videos_doc is None else videos_doc
    videos = {v["id"]: v for v in src["videos"]}
    pred, prev = {}, {}
    for p in results:
        if p["score"] >= threshold and p["video_id"] in videos:
            pred.setdefault(p["video_id"], []).append(p)
    for a in prev_doc["annotations"]:
        prev.setdefault(a["video_id"], []).append(a)
    merged = []
    for vid in list(prev) + [k for k in pred if k not in prev]:
        v = videos[vid]
        H, W, T = v["height"], v["width"], v["length"]
        qs = pred.get(vid, [])
        for e in qs + prev.get(vid, []):
            if len(e["segmentations"]) != T:
                raise ValueError(f"video {vid}: {len(e['segmentations'])} segmentations for {T} frames")
            for s in e["segmentations"]:
                if s is not None and list(s["size"]) != [H, W]:
                    raise ValueError(f"video {vid}: RLE of size {s['size']}")
        for p in qs:
            bb, ar = numpy_bbox_area(p["segmentations"], H, W)
            merged.append({"video_id": vid, "iscrowd": 0, "height": H, "width": W, "length": T, "segmentations": p["segmentations"],
                           "bboxes": bb, "areas": ar, "category_id": p["category_id"], "score": p["score"]})
        for a in prev.get(vid, []):
            if keep_track(a["segmentations"], [p["segmentations"] for p in qs], H, W, frames):
                merged.append(dict(a))
    cats = {c["id"] for c in prev_doc["categories"]}
    for n, a in enumerate(merged):
        if a["category_id"] not in cats:
            raise ValueError(f"video {a['video_id']}: category_id {a['category_id']}")
        a["id"] = n + 1
    doc = {k: src[k] for k in ("info", "licenses") if k in src}
    doc["videos"], doc["categories"], doc["annotations"] = src["videos"], prev_doc["categories"], merged
    return doc


# ------------------------------------------------------------------------------------------------------------------ cases
def _enc(m, k):
    return R.rle_u(m) if k % 3 == 0 else R.rle_c(m)


def _track(H, W, T, rng, absent=(), base=None):
    """T frames of one drifting blob (or of `base` jittered), None at the frames in `absent`"""
    m = R.blob(H, W, rng) if base is None else base
    out = []
    for t in range(T):
        out.append(None if t in absent else _enc(m, t + int(rng.integers(0, 3))))
        m = R.jitter(m, rng) if H > 4 and W > 4 else m
    return out


def _item(vid, H, W, T, dsegs, gsegs):
    return SimpleNamespace(vid=vid, H=H, W=W, T=T, dsegs=dsegs, gsegs=gsegs)


def _pair_track(H, W, frames):
    """frames: per frame (inter, area_p, area_q) or None for a frame without a P-side segmentation (the Q side then has 5 pixels)
    -> (p track, q track) with exactly those counts"""
    p, q = [], []
    for f in frames:
        if f is None:
            p.append(None)
            q.append(R.rle_c(R.pair(H, W, 0, 0, min(5, H * W))[1]))
        else:
            a, b = R.pair(H, W, *f)
            p.append(R.rle_c(a))
            q.append(R.rle_u(b))
    return p, q


# name -> (per-frame counts, kept under `annotated`, kept under `all`).  `half`: 2 * inter == union exactly, dropped; `below`: one
# union pixel more, kept; under `all` the unannotated frame adds the Q side's 5 pixels to the union of both, so both are kept there
NAMED_TUBES = {"half": ([(1, 2, 1), (1, 1, 2), None], False, True), "below": ([(1, 2, 1), (1, 1, 3), None], True, True),
               "half_dense": ([(100, 150, 150), (200, 300, 300)], False, False), "below_dense": ([(100, 150, 150), (200, 300, 301)], True, True)}


def kernel_case():
    """ONE chunk for device_merge: videos of KERNEL_SIZES with T = 1, 2, 5 -> (items, names).  It holds D = 0, G = 0 and both; D = 9
    with G = 17 (two by three pair tiles with ragged edges); None frames on the P side, the Q side and both at the same t; a track
    with no annotated frame; the pairs of NAMED_TUBES"""
    rng = np.random.default_rng(23)
    items, names = [], {}
    one = R.rle_c(np.ones((1, 1), bool))
    items.append(_item(1, 1, 1, 1, [[one]], [[one], [R.rle_c(np.zeros((1, 1), bool))]]))            # identical: dropped
    items.append(_item(2, 5, 7, 2, [], [_track(5, 7, 2, rng), _track(5, 7, 2, rng, absent=(1,))]))   # D == 0
    items.append(_item(3, 5, 7, 5, [_track(5, 7, 5, rng), _track(5, 7, 5, rng, absent=(0, 4))], []))  # G == 0: kept
    items.append(_item(4, 31, 33, 1, [], []))                                                        # neither
    H, W, T = 31, 33, 5
    bases = [R.blob(H, W, rng) for _ in range(6)]
    absent_p = [(), (1,), (0, 2, 4), (0, 1, 2, 3, 4), (3,), (), (1, 2), (4,), (0,)]                  # track 3: no annotated frame
    absent_q = [(), (1,), (2,), (0, 3), ()] + [()] * 4 + [(1, 3)] + [()] * 7                         # t = 1: absent on both sides
    d = [_track(H, W, T, rng, absent=a, base=bases[k % 6]) for k, a in enumerate(absent_p)]
    g = [_track(H, W, T, rng, absent=a, base=bases[(k * 5) % 6] if k % 2 else None) for k, a in enumerate(absent_q)]
    assert len(d) == 9 and len(g) == 17
    items.append(_item(5, H, W, T, d, g))
    names["big"] = 4
    for k, (name, (fr, _, _)) in enumerate(NAMED_TUBES.items()):
        H, W = (64, 64) if k % 2 == 0 else (40, 100)
        p, q = _pair_track(H, W, fr)
        names[name] = len(items)
        items.append(_item(10 + k, H, W, len(fr), [p], [q]))
    H, W = 40, 100
    base = R.blob(H, W, rng)
    items.append(_item(20, H, W, 2, [_track(H, W, 2, rng, base=base), _track(H, W, 2, rng)],
                       [_track(H, W, 2, rng, base=base), _track(H, W, 2, rng), _track(H, W, 2, rng, absent=(0, 1))]))
    items.append(_item(21, 64, 64, 1, [_track(64, 64, 1, rng)], [_track(64, 64, 1, rng)]))
    assert {(it.H, it.W) for it in items} == set(KERNEL_SIZES) and {it.T for it in items} >= {1, 2, 5}
    return items, names


def many_videos(n, seed=3):
    """n small videos with one or two tracks a side: the call-count case"""
    rng = np.random.default_rng(seed)
    return [_item(100 + k, 5, 7, 2, [_track(5, 7, 2, rng) for _ in range(1 + k % 2)], [_track(5, 7, 2, rng) for _ in range(1 + k % 3 // 2)])
            for k in range(n)]


def merge_case(seed=0):
    """a synthetic two-round case of 12 videos -> (round-0 document, results).  Keymask-style previous tracks (a few annotated frames),
    dense predictions that cover some of them, a video with only predictions (id 3), one with only previous tracks (id 4), one
    whose predictions all score below the threshold (id 5), a prediction of a video the file does not have, a score exactly at the
    threshold, and results in an order that is not the videos'"""
    rng = np.random.default_rng(seed)
    sizes = [(24, 40), (31, 33), (40, 100), (20, 24)]
    videos, anns, preds = [], [], []
    for k in range(12):
        vid = 1 + k
        H, W = sizes[k % 4]
        T = (3, 5, 4)[k % 3]
        videos.append({"id": vid, "height": H, "width": W, "length": T, "file_names": [f"v{vid}/{t:05d}.jpg" for t in range(T)]})
        objs = [R.blob(H, W, rng) for _ in range(int(rng.integers(1, 4)))]
        if vid != 3:
            for j, m in enumerate(objs):
                key = sorted(rng.choice(T, size=int(rng.integers(1, min(T, 3) + 1)), replace=False).tolist())
                segs = _track(H, W, T, rng, absent=[t for t in range(T) if t not in key], base=m)
                masks = [None if s is None else R.seg_mask(s, H, W) for s in segs]
                anns.append({"id": 1000 + len(anns), "video_id": vid, "category_id": 1, "iscrowd": 0, "height": H, "width": W, "length": T,
                             "segmentations": segs, "bboxes": [None if m is None else [float(v) for v in R.box_of(m)] for m in masks],
                             "areas": [None if m is None else int(m.sum()) for m in masks]})
        if vid != 4:
            for j in range(int(rng.integers(1, 4))):
                covers = j < len(objs) and rng.random() < 0.7
                segs = _track(H, W, T, rng, absent=(T - 1,) if j == 2 else (), base=objs[j] if covers else None)
                score = 0.75 if (vid, j) == (1, 0) else float(np.round(rng.uniform(0.1, 0.7) if vid == 5 else rng.uniform(0.6, 1.0), 3))
                preds.append({"video_id": vid, "category_id": 1, "score": score, "segmentations": segs})
    preds.append({"video_id": 99, "category_id": 1, "score": 0.99, "segmentations": [None]})                 # no such video: skipped
    order = rng.permutation(len(preds))
    anns = [a for a in anns if a["video_id"] == 7] + [a for a in anns if a["video_id"] != 7]                 # file order is not video order
    doc = {"info": {"description": "round 0"}, "licenses": [], "videos": videos, "annotations": anns,
           "categories": [{"id": 1, "name": "object", "supercategory": "object"}]}
    return doc, [preds[i] for i in order]
