#!/usr/bin/env python3
"""Throughput of the image self-training merge (s2d_amd/selftrain.py) and of the ragged RLE decode under it (csrc/rle_ragged.hip,
s2d_amd/rle_ragged.py) on an ImageNet-shaped synthetic set: 20,000 images of at most 500 x 375, 1-3 previous masks and 0-5 predictions
above the threshold each (plus as many below it), compressed RLE, no `bbox`, fixed seeds.  Masks are rectangles; about half of the
predictions are jittered copies of a previous mask, so kept and dropped previous masks both occur.

In one run, medians of 3 with the two paths alternating:
  (a) decode + tight boxes of every mask of the set, chunked as merge_round chunks them: the ragged path (stage_rle_ragged +
      decode_ragged: 3 library calls per chunk) against the per-image path (coco_eval.decode_segmentations + ytvis_eval.plane_bboxes:
      3 per image), host staging included in both, one device synchronise at the end of each; seconds and library calls.  The boxes
      of the two paths must be equal.
  (b) merge_files on the set: seconds by phase -- stage, decode, iou, keep (device-inclusive), assemble (the host logic), json (reading
      the two files and writing the third) -- and the total.
  (c) the two paths of (a) on the COCO-val-shaped set of scripts/coco_eval_throughput.py (--coco-images of them: around 480 x 640, about
      107 masks each), to size a switch of the evaluator to the ragged decode.

    python scripts/selftrain_throughput.py [--images 20000] [--coco-images 1000] [--limit 1100] [--out profiles/selftrain/throughput.json]

The measurement runs in a child process under a time limit; prints one JSON line.  Progress goes to stderr."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

SIZES = [(375, 500), (500, 375), (333, 500), (500, 333), (375, 500), (281, 500), (400, 500), (500, 400), (250, 333), (224, 224)]


def compress(counts):
    """maskApi.c rleToString of a counts array, vectorised over the counts"""
    import numpy as np
    c = np.asarray(counts, np.int64)
    x = c.copy()
    x[3:] -= c[1:-2]
    out = np.zeros((len(x), 13), np.uint8)
    n = np.zeros(len(x), np.int64)
    more = np.ones(len(x), bool)
    for k in range(13):
        ch = x & 0x1f
        x = x >> 5
        m = np.where(ch & 0x10, x != -1, x != 0)
        out[:, k] = np.where(more, ch | (m.astype(np.int64) << 5), 0) + 48
        n += more
        more &= m
    return out[np.arange(13)[None, :] < n[:, None]].tobytes().decode()


def rect_rle(x, y, w, h, H, W):
    """the compressed COCO RLE of the rectangle [x, x + w) x [y, y + h) in an H x W image (column-major runs)"""
    import numpy as np
    if h == H:
        counts = [x * H, w * H, (W - x - w) * H]
    else:
        counts = np.empty(2 * w + 1, np.int64)
        counts[0] = x * H + y
        counts[1::2] = h
        counts[2::2] = H - h
        counts[-1] = (H - y - h) + (W - x - w) * H
        counts = counts.tolist()
    if counts[-1] == 0:
        counts = counts[:-1]
    return {"size": [H, W], "counts": compress(counts)}


def make_set(n_images, threshold=0.7):
    """-> (previous annotation document, predictions list)"""
    import numpy as np
    rng = np.random.default_rng(1000)
    doc = {"images": [], "annotations": [], "categories": [{"id": 1, "name": "fg", "supercategory": "fg"}]}
    preds = []

    def rect(H, W):
        w, h = int(rng.integers(8, W * 3 // 4)), int(rng.integers(8, H * 3 // 4))
        return int(rng.integers(0, W - w + 1)), int(rng.integers(0, H - h + 1)), w, h

    for n in range(n_images):
        H, W = SIZES[n % len(SIZES)]
        doc["images"].append({"id": n + 1, "height": H, "width": W, "file_name": f"{n + 1:08d}.JPEG"})
        prev = [rect(H, W) for _ in range(int(rng.integers(1, 4)))]
        for r in prev:
            doc["annotations"].append({"id": len(doc["annotations"]) + 1, "image_id": n + 1, "category_id": 1, "iscrowd": 0,
                                       "segmentation": rect_rle(*r, H, W)})
        k = int(rng.integers(0, 6))
        for j in range(2 * k):                                           # k above the threshold, k below
            if rng.random() < 0.5:
                x, y, w, h = prev[j % len(prev)]
                dx, dy = (int(v) for v in rng.integers(-12, 13, 2))
                x, y = min(max(x + dx, 0), W - w), min(max(y + dy, 0), H - h)
                r = (x, y, w, h)
            else:
                r = rect(H, W)
            score = float(np.round(rng.uniform(threshold, 1.0) if j < k else rng.uniform(0.05, threshold - 0.001), 4))
            preds.append({"image_id": n + 1, "category_id": 1, "score": score, "segmentation": rect_rle(*r, H, W)})
    return doc, preds


def _median(xs):
    return sorted(xs)[len(xs) // 2]


def decode_both(images, dev, log, name):
    """images: [(segs, H, W)].  -> the (a) / (c) record: both paths on the same chunks, medians of 3, alternating"""
    import numpy as np
    import torch
    from s2d_amd import coco_eval, rle_ragged
    from s2d_amd.ytvis_eval import plane_bboxes
    chunks, chunk, words = [], [], 0
    for segs, H, W in images:
        w = len(segs) * ((H * W + 31) // 32)
        if chunk and (words + w > coco_eval.CHUNK_WORDS or len(chunk) >= coco_eval.CHUNK_IMAGES):
            chunks.append(chunk)
            chunk, words = [], 0
        chunk.append((segs, H, W))
        words += w
    if chunk:
        chunks.append(chunk)

    def ragged(keep=False):
        before = sum(rle_ragged.LIB_CALLS.values())
        boxes = []
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for c in chunks:
            out = rle_ragged.decode_ragged(rle_ragged.stage_rle_ragged([s for s, _, _ in c], [(H, W) for _, H, W in c]), dev)
            if keep:
                boxes.append(out.bbox)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, sum(rle_ragged.LIB_CALLS.values()) - before, boxes

    def per_image(keep=False):
        before = coco_eval.LIB_CALLS["decode"]
        boxes, calls = [], 0
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for c in chunks:
            for segs, H, W in c:
                b = plane_bboxes(coco_eval.decode_segmentations(segs, H, W, dev), H, W)
                calls += 1 if len(segs) else 0
                if keep:
                    boxes.append(b)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, coco_eval.LIB_CALLS["decode"] - before + calls, boxes

    _, _, a = ragged(keep=True)                                           # warm-up of both, and the equality of what they compute
    _, _, b = per_image(keep=True)
    equal = bool(torch.equal(torch.cat(a), torch.cat(b)))
    del a, b
    tr, tp = [], []
    for _ in range(3):
        s, rc, _ = ragged()
        tr.append(s)
        s, pc, _ = per_image()
        tp.append(s)
    rec = {"images": len(images), "planes": int(sum(len(s) for s, _, _ in images)), "chunks": len(chunks),
           "ragged": {"seconds": round(_median(tr), 4), "all_runs_s": [round(v, 4) for v in tr], "library_calls": rc},
           "per_image": {"seconds": round(_median(tp), 4), "all_runs_s": [round(v, 4) for v in tp], "library_calls": pc},
           "speedup": round(_median(tp) / max(_median(tr), 1e-9), 2), "boxes_equal": equal}
    log(f"{name}: ragged {rec['ragged']} per image {rec['per_image']} equal {equal}")
    return rec


def measure(n_images, coco_images):
    import torch
    from s2d_amd import selftrain

    def log(msg):
        print(f"[{time.perf_counter() - t_start:7.1f} s] {msg}", file=sys.stderr, flush=True)

    t_start = time.perf_counter()
    dev = torch.device("cuda", 0)
    doc, preds = make_set(n_images)
    kept = [p for p in preds if p["score"] >= 0.7]
    res = {"device": torch.cuda.get_device_name(0),
           "set": {"images": n_images, "previous_masks": len(doc["annotations"]), "predictions": len(preds), "kept_predictions": len(kept),
                   "sizes": SIZES, "generate_s": round(time.perf_counter() - t_start, 1)}}
    log(f"set: {res['set']}")
    by = {}
    for e in doc["annotations"] + kept:
        by.setdefault(e["image_id"], []).append(e["segmentation"])
    res["decode_bbox"] = decode_both([(by[im["id"]], im["height"], im["width"]) for im in doc["images"] if im["id"] in by], dev, log, "(a)")

    with tempfile.TemporaryDirectory() as tmp:
        paths = [os.path.join(tmp, n) for n in ("results.json", "round0.json", "round1.json")]
        for p, d in zip(paths, (preds, doc)):
            with open(p, "w") as fh:
                json.dump(d, fh)
        runs = []
        for k in range(4):                                                # the first run warms up
            seconds = {}
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = selftrain.merge_files(*paths, device=dev, seconds=seconds)
            torch.cuda.synchronize()
            seconds["total"] = time.perf_counter() - t0
            if k:
                runs.append(seconds)
        phases = ("stage", "decode", "iou", "keep", "assemble", "json", "total")
        res["merge_files"] = {"seconds": {p: round(_median([r[p] for r in runs]), 4) for p in phases},
                              "all_runs_total_s": [round(r["total"], 4) for r in runs], "annotations_out": len(out["annotations"]),
                              "previous_masks_dropped": len(doc["annotations"]) + len(kept) - len(out["annotations"]),
                              "chunk_images": selftrain.CHUNK_IMAGES}
        log(f"(b): {res['merge_files']}")
    del doc, preds, kept, by

    if coco_images:
        import coco_eval_throughput as C
        cdoc, cres = C.make_set(coco_images, dev, log)
        by = {}
        for e in cres + cdoc["annotations"]:
            by.setdefault(e["image_id"], []).append(e["segmentation"])
        res["decode_bbox_coco_val_shaped"] = decode_both([(by[im["id"]], im["height"], im["width"]) for im in cdoc["images"]], dev, log, "(c)")
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=20000)
    ap.add_argument("--coco-images", type=int, default=1000, help="images of the COCO-val-shaped set of (c); 0 leaves (c) out")
    ap.add_argument("--limit", type=int, default=1100, help="seconds for the measuring child process")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        print(json.dumps(measure(a.images, a.coco_images)), flush=True)
        return 0
    t0 = time.perf_counter()
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--images", str(a.images), "--coco-images", str(a.coco_images)],
                           stdout=subprocess.PIPE, text=True, timeout=a.limit, cwd=ROOT)
    except subprocess.TimeoutExpired:
        print(f"the measurement exceeded {a.limit} s", file=sys.stderr)
        return 1
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    if r.returncode != 0 or not lines:
        print(f"the measurement failed with status {r.returncode}", file=sys.stderr)
        return 1
    res = json.loads(lines[-1])
    res["script_s"] = round(time.perf_counter() - t0, 1)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
