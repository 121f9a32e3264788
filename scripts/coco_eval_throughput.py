#!/usr/bin/env python3
"""Throughput of the COCO image evaluator (csrc/coco_eval.hip, s2d_amd/coco_eval.py) on a COCO-val-shaped synthetic set: 5000
images around 480 x 640, 100 detections each (compressed RLE + box), ground-truth counts 1 + Poisson(6) (mean about 7, compressed
RLE + `area` + `bbox`), about 3 % crowds, fixed seeds.  Masks are rectangles: the first detections are jittered copies of the
ground truths, the rest are random, so matches, misses, ties at IoU 1 and crowd hits all occur.

For both iou types, in one run: evaluate_coco with the device matcher and with matcher="host" (the Python loop on the same
device-computed IoUs), each with profile=True -- seconds split into decode (RLE parse + decode, per image), iou (one ragged launch
per chunk + the copy back), match (group tables + the matching launch, or the Python loop) and accumulate -- and the number of
library calls of each kind; the two matchers' stats must be equal.  --host-images N runs the host matcher on the first N images
only (both paths are then also timed on that subset, so that the pair is comparable).

    python scripts/coco_eval_throughput.py [--images 5000] [--host-images 5000] [--limit 1100] [--out profiles/coco_eval/throughput.json]

The measurement runs in a child process under a time limit; prints one JSON line.  Progress goes to stderr."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = [(480, 640), (427, 640), (640, 480), (500, 375), (375, 500), (480, 640), (640, 427), (428, 640)]
DETS = 100


def _rects(rng, n, H, W):
    import numpy as np
    w = np.minimum(np.maximum((rng.lognormal(4.0, 0.9, n)).astype(np.int64), 4), W - 1)
    h = np.minimum(np.maximum((rng.lognormal(4.0, 0.9, n)).astype(np.int64), 4), H - 1)
    x = (rng.random(n) * (W - w)).astype(np.int64)
    y = (rng.random(n) * (H - h)).astype(np.int64)
    return np.stack([x, y, w, h], 1)


def make_set(n_images, dev, log):
    """-> (COCO document, results list)"""
    import numpy as np
    import torch
    from s2d_amd.rle import encode_video_predictions
    rng = np.random.default_rng(2017)
    doc = {"images": [], "annotations": [], "categories": [{"id": 1, "name": "fg"}]}
    results = []
    for n in range(n_images):
        H, W = SIZES[n % len(SIZES)]
        G = 1 + int(rng.poisson(6.0))
        g = _rects(rng, G, H, W)
        d = _rects(rng, DETS, H, W)
        k = min(G, DETS)
        jit = rng.integers(-6, 7, (k, 4))
        jit[rng.random(k) < 0.2] = 0                                        # exact copies: IoU 1
        d[:k] = g[:k] + jit
        d[:, 2:] = np.maximum(d[:, 2:], 2)
        d[:, 0] = np.clip(d[:, 0], 0, W - 2); d[:, 1] = np.clip(d[:, 1], 0, H - 2)
        d[:, 2] = np.minimum(d[:, 2], W - d[:, 0]); d[:, 3] = np.minimum(d[:, 3], H - d[:, 1])
        b = torch.from_numpy(np.concatenate([d, g])).to(dev)
        yy = torch.arange(H, device=dev)[None, :, None]
        xx = torch.arange(W, device=dev)[None, None, :]
        m = ((xx >= b[:, 0, None, None]) & (xx < (b[:, 0] + b[:, 2])[:, None, None]) & (yy >= b[:, 1, None, None])
             & (yy < (b[:, 1] + b[:, 3])[:, None, None])).to(torch.uint8)
        segs = encode_video_predictions(m[:, None].contiguous())
        scores = np.round(rng.random(DETS), 4)
        doc["images"].append({"id": n + 1, "height": H, "width": W, "file_name": f"{n + 1:012d}.jpg"})
        for i in range(DETS):
            s = segs[i][0]
            results.append({"image_id": n + 1, "category_id": 1, "score": float(scores[i]), "bbox": [float(v) for v in d[i]],
                            "segmentation": dict(s, counts=s["counts"].decode() if isinstance(s["counts"], bytes) else s["counts"])})
        for j in range(G):
            s = segs[DETS + j][0]
            doc["annotations"].append({"id": len(doc["annotations"]) + 1, "image_id": n + 1, "category_id": 1,
                                       "iscrowd": int(rng.random() < 0.03), "area": float(g[j, 2] * g[j, 3]), "bbox": [float(v) for v in g[j]],
                                       "segmentation": dict(s, counts=s["counts"].decode() if isinstance(s["counts"], bytes) else s["counts"])})
        if (n + 1) % 500 == 0:
            log(f"generated {n + 1} images")
    return doc, results


def measure(n_images, host_images):
    import numpy as np
    import torch
    from s2d_amd.coco_eval import evaluate_coco

    def log(msg):
        print(f"[{time.perf_counter() - t_start:7.1f} s] {msg}", file=sys.stderr, flush=True)

    t_start = time.perf_counter()
    dev = torch.device("cuda", 0)
    doc, results = make_set(n_images, dev, log)
    res = {"device": torch.cuda.get_device_name(0),
           "set": {"images": n_images, "detections": len(results), "ground_truths": len(doc["annotations"]),
                   "mean_ground_truths": round(len(doc["annotations"]) / n_images, 3), "crowds": sum(a["iscrowd"] for a in doc["annotations"]),
                   "sizes": SIZES, "generate_s": round(time.perf_counter() - t_start, 1)}}
    if host_images < n_images:
        keep = {im["id"] for im in doc["images"][:host_images]}
        sub = {"images": doc["images"][:host_images], "categories": doc["categories"],
               "annotations": [a for a in doc["annotations"] if a["image_id"] in keep]}
        sub_results = [r for r in results if r["image_id"] in keep]
    else:
        sub, sub_results = doc, results
    nw = min(50, n_images)                                                  # warm-up: library load, allocator
    evaluate_coco({"images": doc["images"][:nw], "categories": doc["categories"],
                   "annotations": [a for a in doc["annotations"] if a["image_id"] <= nw]},
                  [r for r in results if r["image_id"] <= nw], device=dev)

    def run(d, r, iou_type, matcher):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ev = evaluate_coco(d, r, iou_type=iou_type, device=dev, matcher=matcher, profile=True)
        total = time.perf_counter() - t0
        stats = ev.summarize(out=None)
        out = {"images": len(d["images"]), "total_s": round(total, 3), "seconds": {k: round(ev.seconds[k], 3) for k in ("decode", "iou", "match", "accumulate")},
               "library_calls": dict(ev.launches), "AP": round(float(stats[0]), 6), "AR100": round(float(stats[8]), 6)}
        log(f"{iou_type} {matcher} on {len(d['images'])} images: {out['total_s']} s {out['seconds']}")
        return out, stats

    for t in ("segm", "bbox"):
        full, _ = run(doc, results, t, "device")
        dev_sub, s_dev = (full, _) if sub is doc else run(sub, sub_results, t, "device")
        host, s_host = run(sub, sub_results, t, "host")
        res[t] = {"device_matcher": full, "host_matcher": host, "stats_equal": bool(np.array_equal(s_dev, s_host)),
                  "match_speedup_same_images": round(host["seconds"]["match"] / max(dev_sub["seconds"]["match"], 1e-9), 1)}
        if sub is not doc:
            res[t]["device_matcher_on_host_subset"] = dev_sub
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=5000)
    ap.add_argument("--host-images", type=int, default=None, help="images the host matcher runs on (default: all)")
    ap.add_argument("--limit", type=int, default=1100, help="seconds for the measuring child process")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    host_images = a.images if a.host_images is None else min(a.host_images, a.images)
    if a.child:
        print(json.dumps(measure(a.images, host_images)), flush=True)
        return 0
    t0 = time.perf_counter()
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--images", str(a.images), "--host-images", str(host_images)],
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
