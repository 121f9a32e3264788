#!/usr/bin/env python3
"""Throughput of the video self-training merge (s2d_amd/selftrain_video.py, csrc/selftrain_video.hip) on two synthetic sets, fixed
seeds, masks are moving rectangles in compressed RLE:

  ytvis   --ytvis-videos videos of 20-36 frames at 720 x 1280; 1-3 previous tracks each, keymask style (1-3 annotated frames, the
          rest None); 1-4 predictions above the threshold (about half of them follow a previous track) and one below it;
  davis   --davis-videos videos of 70-100 frames at 480 x 854; 1-3 previous tracks annotated on EVERY frame, 1-3 predictions.

On each set, in one run, medians of 3 with the paths alternating, host staging included, one device synchronise at the end of each:
  (a) the chunked path: selftrain_video.device_merge over the chunks merge_round forms (decode + boxes + areas + tube counts + keep,
      one read-back per chunk), timed under --frames annotated and under --frames all;
  (b) today's per-item pattern: keymask.results_to_annotations.device_bboxes_areas per kept prediction, plus per video with both
      kinds of track two ytvis_eval.decode_frames and one ytvis_eval.video_ious (the all-frame IoU) with the 0.5 rule on the host.
Seconds and library calls of each; the boxes and areas of the two paths must be equal, and the keep flags of (a) under `all` must
equal (b)'s.  Then merge_files on the set under the default frame set: seconds by phase -- stage, decode, counts, keep
(device-inclusive), assemble (host logic), json -- and the total.

    python scripts/selftrain_video_throughput.py [--ytvis-videos 2000] [--davis-videos 30] [--limit 1100] [--out profiles/selftrain_video/throughput.json]

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


def make_set(kind, n_videos, threshold=0.75):
    """-> (previous annotation document, results list)"""
    import numpy as np
    from selftrain_throughput import rect_rle
    rng = np.random.default_rng(2000 if kind == "ytvis" else 3000)
    H, W = (720, 1280) if kind == "ytvis" else (480, 854)
    doc = {"info": {}, "licenses": [], "videos": [], "annotations": [], "categories": [{"id": 1, "name": "object", "supercategory": "object"}]}
    preds = []

    def path(T):
        """a rectangle that drifts: [(x, y, w, h)] per frame"""
        w, h = int(rng.integers(40, W // 3)), int(rng.integers(40, H // 2))
        x, y = float(rng.integers(0, W - w + 1)), float(rng.integers(0, H - h + 1))
        vx, vy = rng.uniform(-6, 6, 2)
        out = []
        for _ in range(T):
            out.append((int(min(max(x, 0), W - w)), int(min(max(y, 0), H - h)), w, h))
            x, y = x + vx, y + vy
        return out

    def track(p, absent=(), dx=0, dy=0):
        return [None if t in absent else rect_rle(min(max(x + dx, 0), W - w), min(max(y + dy, 0), H - h), w, h, H, W)
                for t, (x, y, w, h) in enumerate(p)]

    for n in range(n_videos):
        T = int(rng.integers(20, 37)) if kind == "ytvis" else int(rng.integers(70, 101))
        doc["videos"].append({"id": n + 1, "height": H, "width": W, "length": T, "file_names": [f"{n + 1:05d}/{t:05d}.jpg" for t in range(T)]})
        paths = [path(T) for _ in range(int(rng.integers(1, 4)))]
        for p in paths:
            key = set(rng.choice(T, size=int(rng.integers(1, 4)), replace=False).tolist()) if kind == "ytvis" else set(range(T))
            segs = track(p, absent=[t for t in range(T) if t not in key])
            doc["annotations"].append({"id": len(doc["annotations"]) + 1, "video_id": n + 1, "category_id": 1, "iscrowd": 0, "height": H,
                                       "width": W, "length": T, "segmentations": segs, "bboxes": [None if s is None else [0.0, 0.0, 1.0, 1.0] for s in segs],
                                       "areas": [None if s is None else 1 for s in segs]})
        k = int(rng.integers(1, 5 if kind == "ytvis" else 4))
        for j in range(k + 1):                                            # k above the threshold, one below
            if rng.random() < 0.5:
                segs = track(paths[j % len(paths)], dx=int(rng.integers(-8, 9)), dy=int(rng.integers(-8, 9)))
            else:
                segs = track(path(T))
            score = float(np.round(rng.uniform(threshold, 1.0) if j < k else rng.uniform(0.05, threshold - 0.001), 4))
            preds.append({"video_id": n + 1, "category_id": 1, "score": score, "segmentations": segs})
    return doc, preds


def _median(xs):
    return sorted(xs)[len(xs) // 2]


class CallCounter:
    """counts every library call made through s2d_amd._lib.lib().call"""

    def __init__(self):
        from s2d_amd._lib import lib
        self.n = 0
        L = lib()
        inner = L.call

        def call(name, *args):
            self.n += 1
            return inner(name, *args)
        L.call = call


def measure_set(kind, n_videos, log):
    import numpy as np
    import torch
    from s2d_amd import selftrain_video as S, ytvis_eval
    from s2d_amd.keymask.results_to_annotations import device_bboxes_areas
    dev = torch.device("cuda", 0)
    t0 = time.perf_counter()
    doc, preds = make_set(kind, n_videos)
    items = S.plan_round(doc, preds)
    chunks = list(S._chunks(items))
    work = [it for it in items if it.gsegs]
    rec = {"videos": n_videos, "size": [doc["videos"][0]["height"], doc["videos"][0]["width"]],
           "frames": [min(v["length"] for v in doc["videos"]), max(v["length"] for v in doc["videos"])],
           "previous_tracks": len(doc["annotations"]), "predictions": len(preds), "kept_predictions": sum(len(it.gsegs) for it in work),
           "planes_decoded": sum((len(it.dsegs) + len(it.gsegs)) * it.T for it in work), "chunks": len(chunks),
           "slabbed_chunks": sum(bool(c.slabs) for c in chunks), "generate_s": round(time.perf_counter() - t0, 1)}
    log(f"{kind} set: {rec}")
    counter = CallCounter()

    def chunked(frames, keep=False):
        n0, out = counter.n, []
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for c in chunks:
            r = S.device_merge(c, frames, dev)
            if keep:
                out.append(r)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, counter.n - n0, out

    def per_item(keep=False):
        n0, flags, areas, boxes = counter.n, [], [], []
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for it in work:
            for segs in it.gsegs:
                bb, ar = device_bboxes_areas(segs, it.H, it.W)
                if keep:
                    boxes += bb
                    areas += ar
            if it.dsegs:
                D, G = len(it.dsegs), len(it.gsegs)
                db = ytvis_eval.decode_frames([s for tr in it.dsegs for s in tr], it.H, it.W, device=dev)
                gb = ytvis_eval.decode_frames([s for tr in it.gsegs for s in tr], it.H, it.W, device=dev)
                ious, _ = ytvis_eval.video_ious(db, D, gb, G, it.T)
                flags += (ious < 0.5).all(axis=1).tolist()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, counter.n - n0, (flags, areas, boxes)

    _, _, a = chunked("all", keep=True)                                   # warm-up of both, and the equality of what they compute
    _, _, (flags, areas, boxes) = per_item(keep=True)
    got_keep = np.concatenate([r[0] for r in a]).astype(bool).tolist()
    got_areas = np.concatenate([r[1] for r in a]).tolist()
    got_boxes = np.concatenate([r[2] for r in a]).astype(np.float64).tolist()
    # (b) writes None for an absent frame; the rectangles here are dense on the prediction side
    rec["equal"] = {"keep_all_frames": got_keep == flags, "areas": got_areas == areas, "boxes": got_boxes == boxes}
    del a, flags, areas, boxes
    chunked("annotated")
    ta, tl, tb = [], [], []
    for _ in range(3):
        s, ca, _ = chunked("annotated")
        ta.append(s)
        s, cl, _ = chunked("all")
        tl.append(s)
        s, cb, _ = per_item()
        tb.append(s)
    rec["chunked_annotated"] = {"seconds": round(_median(ta), 4), "all_runs_s": [round(v, 4) for v in ta], "library_calls": ca}
    rec["chunked_all"] = {"seconds": round(_median(tl), 4), "all_runs_s": [round(v, 4) for v in tl], "library_calls": cl}
    rec["per_item"] = {"seconds": round(_median(tb), 4), "all_runs_s": [round(v, 4) for v in tb], "library_calls": cb}
    rec["speedup_all"] = round(_median(tb) / max(_median(tl), 1e-9), 2)
    rec["speedup_annotated"] = round(_median(tb) / max(_median(ta), 1e-9), 2)
    log(f"{kind}: annotated {rec['chunked_annotated']} all {rec['chunked_all']} per item {rec['per_item']} equal {rec['equal']}")

    with tempfile.TemporaryDirectory() as tmp:
        paths = [os.path.join(tmp, n) for n in ("results.json", "round0.json", "round1.json")]
        for p, d in zip(paths, (preds, doc)):
            with open(p, "w") as fh:
                json.dump(d, fh)
        rec["json_bytes"] = sum(os.path.getsize(p) for p in paths[:2])
        runs = []
        for k in range(4):                                                # the first run warms up
            seconds = {}
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = S.merge_files(*paths, device=dev, seconds=seconds)
            torch.cuda.synchronize()
            seconds["total"] = time.perf_counter() - t0
            if k:
                runs.append(seconds)
        phases = ("stage", "decode", "counts", "keep", "assemble", "json", "total")
        rec["merge_files"] = {"seconds": {p: round(_median([r.get(p, 0.0) for r in runs]), 4) for p in phases},
                              "all_runs_total_s": [round(r["total"], 4) for r in runs], "annotations_out": len(out["annotations"]),
                              "previous_tracks_dropped": len(doc["annotations"]) + rec["kept_predictions"] - len(out["annotations"])}
        log(f"{kind} merge_files: {rec['merge_files']}")
    return rec


def measure(ytvis_videos, davis_videos):
    import torch
    t_start = time.perf_counter()

    def log(msg):
        print(f"[{time.perf_counter() - t_start:7.1f} s] {msg}", file=sys.stderr, flush=True)

    res = {"device": torch.cuda.get_device_name(0)}
    if davis_videos:
        res["davis_shaped"] = measure_set("davis", davis_videos, log)
    if ytvis_videos:
        res["ytvis_shaped"] = measure_set("ytvis", ytvis_videos, log)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ytvis-videos", type=int, default=2000)
    ap.add_argument("--davis-videos", type=int, default=30)
    ap.add_argument("--limit", type=int, default=1100, help="seconds for the measuring child process")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        print(json.dumps(measure(a.ytvis_videos, a.davis_videos)), flush=True)
        return 0
    t0 = time.perf_counter()
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--ytvis-videos", str(a.ytvis_videos), "--davis-videos",
                            str(a.davis_videos)], stdout=subprocess.PIPE, text=True, timeout=a.limit, cwd=ROOT)
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
