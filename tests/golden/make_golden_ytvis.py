"""Golden fixture of the YTVIS evaluator (tests/golden/ytvis_eval.json): the reference's own YTVOS / YTVOSeval
(model_training/mask2former_video/data_video/datasets/ytvis_api/ytvos.py, ytvoseval.py), loaded unmodified where they lie,
score a synthetic ground truth and result list built here.

pycocotools is not installed: `pycocotools.mask` is stood in for by name with the RLE primitives the two files call -- area,
merge, toBbox, frPyObjects (uncompressed counts) and decode -- restated on numpy planes (compressed strings decoded by
oracle_np.rle_decode, cached).  Parity is therefore pinned to the reference's evaluation logic (IoU accumulation, matching,
accumulate, summarize), with the RLE primitives restated, as for the encoder.

    python tests/golden/make_golden_ytvis.py          (needs the reference tree; never runs on the GPU box)
"""
import base64
import copy
import importlib.util
import io
import json
import os
import sys
import types
from contextlib import redirect_stdout

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import _ref_shim as R  # noqa: E402
from oracle import oracle_np as O  # noqa: E402
from s2d_amd.rle import strings_from_runs  # noqa: E402

API = os.path.join(R.MT, "mask2former_video", "data_video", "datasets", "ytvis_api")
OUT = os.path.join(HERE, "ytvis_eval.json")


# ------------------------------------------------------------------------------------------ pycocotools.mask stand-in
_cache = {}


def _plane(rle):
    if "_m" in rle:
        return rle["_m"]
    c = rle["counts"]
    key = (tuple(rle["size"]), c if isinstance(c, (str, bytes)) else tuple(c))
    if key not in _cache:
        if isinstance(c, list):
            _cache[key] = _from_counts(c, *rle["size"])
        else:
            _cache[key] = O.rle_decode(rle).astype(bool)
    return _cache[key]


def _from_counts(counts, h, w):
    vals = np.arange(len(counts)) & 1
    return np.repeat(vals, counts).astype(bool).reshape(w, h).T


def _stand_in():
    pm = types.ModuleType("pycocotools.mask")

    def area(r):
        if isinstance(r, list):
            return np.array([area(x) for x in r], np.uint32)
        return np.uint32(_plane(r).sum())

    def merge(rles, intersect=False):
        ms = [_plane(r) for r in rles]
        m = ms[0].copy()
        for x in ms[1:]:
            m = (m & x) if intersect else (m | x)
        return {"size": list(rles[0]["size"]), "_m": m}

    def fr_py_objects(obj, h, w):
        if isinstance(obj, list):
            raise NotImplementedError("polygons")
        return {"size": [h, w], "_m": _from_counts(obj["counts"], h, w)}

    pm.area = area
    pm.merge = merge
    pm.frPyObjects = fr_py_objects
    pm.decode = lambda r: _plane(r).astype(np.uint8)
    pm.toBbox = lambda r: np.asarray(O.rle_area_bbox(_plane(r))[1], np.float64)
    pk = types.ModuleType("pycocotools")
    pk.mask = pm
    sys.modules["pycocotools"], sys.modules["pycocotools.mask"] = pk, pm
    for name in ("matplotlib", "matplotlib.pyplot", "matplotlib.collections", "matplotlib.patches"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules["matplotlib.collections"].PatchCollection = None
    sys.modules["matplotlib.patches"].Polygon = None


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(API, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ------------------------------------------------------------------------------------------ synthetic case
def _rle_runs(m):
    flat = np.asarray(m, bool).T.reshape(-1)
    pos = np.flatnonzero(np.diff(np.concatenate([[False], flat]).astype(np.int8)))
    bounds = np.concatenate([[0], pos, [flat.size]])
    return np.diff(bounds)


def compressed(m):
    runs = _rle_runs(m)
    s = strings_from_runs(runs.astype(np.int64), np.array([0, len(runs)], np.int64))[0]
    return {"size": list(m.shape), "counts": s.decode()}


def uncompressed(m):
    return {"size": list(m.shape), "counts": [int(c) for c in _rle_runs(m)]}


def rect(H, W, y0, x0, h, w):
    m = np.zeros((H, W), bool)
    m[y0:y0 + h, x0:x0 + w] = True
    return m


def build_case():
    rng = np.random.default_rng(11)
    videos, anns, results = [], [], []
    ann_id = [100]

    def gt(vid, cat, frames, enc, areas=None, **extra):
        a = {"id": ann_id[0], "video_id": vid, "category_id": cat, "iscrowd": 0, "segmentations": [], "areas": [], "bboxes": []}
        ann_id[0] += 1
        for t, m in enumerate(frames):
            if m is None:
                a["segmentations"].append(None); a["areas"].append(None); a["bboxes"].append(None)
            else:
                a["segmentations"].append(enc(m)); a["areas"].append(int(m.sum())); a["bboxes"].append(O.rle_area_bbox(m)[1])
        if areas is not None:
            a["areas"] = areas
        a.update(extra)
        anns.append(a)

    def dt(vid, cat, score, frames):
        results.append({"video_id": vid, "score": float(score), "category_id": cat, "segmentations": [compressed(m) for m in frames]})

    def rand_rect(H, W, lo=20, hi=120):
        h, w = rng.integers(lo, hi, 2)
        return int(rng.integers(0, H - h)), int(rng.integers(0, W - w)), int(h), int(w)

    # video 1: compressed gt, a None frame, JSON areas that disagree with the mask; IoU exactly 1/2
    H, W, T = 256, 288, 3
    videos.append({"id": 1, "height": H, "width": W, "length": T})
    g1 = [rect(H, W, 40, 40, 60, 80)] * T
    gt(1, 1, g1, compressed)
    g2 = [rect(H, W, 150, 150, 50, 50), None, rect(H, W, 150, 160, 50, 50)]
    gt(1, 2, g2, compressed, areas=[2500, None, 9999])
    dt(1, 1, 0.9, [rect(H, W, 40, 40, 60, 40)] * T)                # half of g1 in every frame: IoU = 1/2
    dt(1, 2, 0.8, [rect(H, W, 150, 150, 50, 50)] * T)
    dt(1, 1, 0.3, [rect(H, W, *rand_rect(H, W)) for _ in range(T)])
    dt(1, 2, 0.8, [rect(H, W, 160, 150, 40, 50)] * T)               # tied score

    # video 2: > 100 detections (truncation), tied scores, uncompressed gt, an iscrowd gt
    T = 2
    videos.append({"id": 2, "height": H, "width": W, "length": T})
    gts2 = []
    for k in range(3):
        y0, x0, h, w = rand_rect(H, W, 40, 100)
        gts2.append((y0, x0, h, w))
        gt(2, 1 + (k % 2), [rect(H, W, y0, x0, h, w)] * T, uncompressed, iscrowd=1 if k == 2 else 0)
    for n in range(112):
        if n % 9 == 0:
            y0, x0, h, w = gts2[(n // 9) % 3]
            y0, x0 = min(y0 + int(rng.integers(0, 8)), H - h), min(x0 + int(rng.integers(0, 8)), W - w)
        else:
            y0, x0, h, w = rand_rect(H, W)
        dt(2, 1 + int(rng.integers(0, 2)), round(float(rng.uniform(0.05, 0.95)), 2), [rect(H, W, y0, x0, h, w)] * T)

    # video 3: H*W not a multiple of 32; `ignore: 1` without iscrowd (overwritten to 0); an empty-mask detection
    H3, W3, T = 257, 291, 4
    videos.append({"id": 3, "height": H3, "width": W3, "length": T})
    gt(3, 1, [rect(H3, W3, 10, 17, 90, 70 + t) for t in range(T)], compressed, ignore=1)
    gt(3, 2, [None, rect(H3, W3, 120, 200, 100, 91), rect(H3, W3, 121, 200, 100, 91), None], uncompressed)
    dt(3, 1, 0.7, [rect(H3, W3, 10, 17, 90, 70) for t in range(T)])
    dt(3, 2, 0.6, [np.zeros((H3, W3), bool)] * T)
    dt(3, 2, 0.5, [rect(H3, W3, 120, 200, 100, 91)] * T)
    dt(3, 1, 0.4, [rect(H3, W3, 200, 0, 57, 30)] * T)

    # video 4: ground truth and no detections
    T = 2
    videos.append({"id": 4, "height": H, "width": W, "length": T})
    gt(4, 2, [rect(H, W, 30, 30, 40, 40)] * T, compressed)

    # video 5: a large object (> 256^2 average), IoU exactly 3/4
    H5, W5, T = 300, 320, 3
    videos.append({"id": 5, "height": H5, "width": W5, "length": T})
    gt(5, 1, [rect(H5, W5, 10, 10, 280, 300)] * T, compressed)
    gt(5, 2, [rect(H5, W5, 0, 0, 20, 20)] * T, compressed)
    dt(5, 1, 0.95, [rect(H5, W5, 10, 10, 210, 300)] * T)           # 3/4 of the large gt
    dt(5, 2, 0.35, [rect(H5, W5, 0, 0, 20, 10)] * T)
    dt(5, 1, 0.2, [rect(H5, W5, 0, 0, 20, 20)] * T)

    # video 6: medium objects of both categories, a crowd region
    T = 3
    videos.append({"id": 6, "height": H, "width": W, "length": T})
    gt(6, 1, [rect(H, W, 20, 20, 150, 150)] * T, compressed)
    gt(6, 2, [rect(H, W, 180, 180, 60, 100)] * T, uncompressed, iscrowd=1)
    dt(6, 1, 0.85, [rect(H, W, 25, 20, 150, 150)] * T)
    dt(6, 2, 0.75, [rect(H, W, 180, 180, 60, 50)] * T)
    dt(6, 2, 0.74, [rect(H, W, 180, 230, 60, 50)] * T)
    dt(6, 1, 0.10, [rect(H, W, 180, 180, 60, 100)] * T)

    cats = [{"id": 1, "name": "a", "supercategory": "x"}, {"id": 2, "name": "b", "supercategory": "x"}]
    doc = {"info": {}, "licenses": [], "videos": videos, "categories": cats, "annotations": anns}
    for r in results:                                            # the stand-in and the oracle agree on the strings
        for s in r["segmentations"][:1]:
            assert O.rle_decode(s).sum() == _plane(s).sum()
    return doc, results


# ------------------------------------------------------------------------------------------ reference runs
def _pack(a):
    """exact float64 array as unique values + uint16 indices (keeps the fixture small)"""
    a = np.asarray(a, np.float64)
    vals, idx = np.unique(a, return_inverse=True)
    return {"shape": list(a.shape), "values": vals.tolist(),
            "index": base64.b64encode(idx.astype(np.uint16).reshape(-1).tobytes()).decode()}


def run_reference(doc, results, use_cats, max_dets=(1, 10, 100)):
    ytvos, ytvoseval = _load("ytvos"), _load("ytvoseval")
    with redirect_stdout(io.StringIO()) as out:
        gt = ytvos.YTVOS()
        gt.dataset = copy.deepcopy(doc)
        gt.createIndex()
        dt = gt.loadRes(copy.deepcopy(results))
        ev = ytvoseval.YTVOSeval(gt, dt)
        ev.params.maxDets = list(max_dets)
        ev.params.useCats = use_cats
        ev.evaluate()
        if max_dets[-1] <= 100:
            ev.accumulate()
            ev.summarize()
    return ev, dt, out.getvalue()


def main():
    R.install()
    _stand_in()
    doc, results = build_case()
    fx = {"gt": doc, "results": results}
    for uc in (0, 1):
        ev, dt, text = run_reference(doc, results, uc)
        ious = [{"video_id": int(v), "category_id": int(c), "ious": (m.tolist() if len(m) else [])} for (v, c), m in ev.ious.items()]
        evs = []
        for e in ev.evalImgs:
            if e is None:
                evs.append(None)
                continue
            evs.append({"video_id": int(e["video_id"]), "category_id": int(e["category_id"]), "aRng": e["aRng"], "maxDet": e["maxDet"],
                        "dtIds": e["dtIds"], "gtIds": e["gtIds"], "dtScores": e["dtScores"],
                        "dtMatches": e["dtMatches"].astype(np.int64).tolist(), "gtMatches": e["gtMatches"].astype(np.int64).tolist(),
                        "dtIgnore": e["dtIgnore"].astype(np.int64).tolist(), "gtIgnore": np.asarray(e["gtIgnore"]).astype(np.int64).tolist(),
                        "shapes": [list(e["dtMatches"].shape), list(e["gtMatches"].shape)]})
        fx[f"use_cats_{uc}"] = {"ious": ious, "eval_vids": evs, "precision": _pack(ev.eval["precision"]), "recall": _pack(ev.eval["recall"]),
                                "stats": ev.stats.tolist(), "summary": text.split("DONE")[-1].split("\n", 1)[-1]}
        if uc == 0:
            fx["dt_avg_area"] = {str(a["id"]): float(a["avg_area"]) for a in dt.dataset["annotations"]}
    # every detection against every ground truth of its video (maxDets large): the host stage's input in the CPU test
    ev, _, _ = run_reference(doc, results, 0, (1, 10, 100000))
    full = []
    for v in ev.params.vidIds:
        dts = [d for c in ev.params.catIds for d in ev._dts[v, c]]
        gts = [g for c in ev.params.catIds for g in ev._gts[v, c]]
        order = np.argsort([-d["score"] for d in dts], kind="mergesort")
        m = ev.ious[v, -1]
        full.append({"video_id": int(v), "dt_ids": [dts[i]["id"] for i in order], "gt_ids": [g["id"] for g in gts],
                     "ious": m.tolist() if len(m) else []})
    fx["full_ious"] = full
    with open(OUT, "w") as fh:
        json.dump(fx, fh, separators=(",", ":"))
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
