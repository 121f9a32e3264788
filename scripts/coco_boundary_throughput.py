#!/usr/bin/env python3
"""Throughput of COCO Boundary AP (s2d_amd/coco_eval.py, csrc/mask_boundary.hip erode_ragged_kernel) on two synthetic sets made
by the generator of scripts/coco_eval_throughput.py: the COCO-val-shaped one (5000 images around 480 x 640, 100 detections each) and
a many-small-images one (20000 images of at most 160 x 160, 5 detections each).

In one run, per set:
  * evaluate_coco with iou_type "segm" and "boundary", profile=True, alternating, `--repeats` times each after a warm-up:
    seconds by phase (decode, iou, boundary, match, accumulate) -- median, min and max over the repeats;
  * the band phase alone, two ways on the same planes, chunk by chunk as the evaluator cuts the set: the ragged call (one per
    chunk) and ytvis_eval.boundary_planes per image (the only way there was before the ragged kernel: the baseline).  Both are timed
    by a host clock around work that ends in a device synchronise, alternating inside every chunk, `--repeats` times; the sums over
    the chunks are reported per repeat, with median, min and max, and the outputs are compared bitwise.
No ratio is fixed in advance: the JSON holds both times and their spread, and `ragged_slower_beyond_spread` says whether the
ragged call's fastest repeat is slower than the per-image path's slowest one.

    python scripts/coco_boundary_throughput.py [--images 5000] [--small-images 20000] [--repeats 3] [--out profiles/coco_boundary/throughput.json]

The measurement runs in a child process under a time limit; prints one JSON line.  Progress goes to stderr."""
import argparse
import importlib.util
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SMALL_SIZES = [(120, 160), (160, 120), (96, 128), (128, 128), (100, 150), (150, 100), (64, 96), (160, 160)]
SMALL_DETS = 5
PHASES = ("decode", "iou", "boundary", "match", "accumulate")


def _generator():
    spec = importlib.util.spec_from_file_location("coco_eval_throughput", os.path.join(ROOT, "scripts", "coco_eval_throughput.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _spread(values):
    return {"median": round(statistics.median(values), 4), "min": round(min(values), 4), "max": round(max(values), 4),
            "repeats": [round(v, 4) for v in values]}


def band_phase(doc, results, dev, repeats, ratio=0.02):
    """the bands of every plane of the set, chunk by chunk, timed both ways -> dict"""
    import numpy as np
    import torch
    from s2d_amd import coco_eval as ce
    from s2d_amd.ytvis_eval import boundary_dilation, boundary_planes
    gt = ce.COCOGroundTruth(doc)
    by_img = {}
    for n, r in enumerate(results):
        by_img.setdefault(r["image_id"], []).append(n)
    ragged, per_image = [0.0] * repeats, [0.0] * repeats
    chunks = planes = words_total = 0
    equal = True

    def run(chunk):
        nonlocal chunks, planes, words_total, equal
        bits = [ce.decode_segmentations(segs, H, W, dev) for segs, H, W in chunk]
        st = ce.stage_planes([(b, None, H, W) for b, (_, H, W) in zip(bits, chunk)], [[] for _ in chunk], dev)
        spec = np.array([[st.img[n, 0], len(b), H, W, boundary_dilation(H, W, ratio)] for n, (b, (_, H, W)) in enumerate(zip(bits, chunk))],
                        np.int64)
        out = torch.empty_like(st.bits)
        for rep in range(-1, repeats):                                         # -1: warm-up of both ways on this chunk's shapes
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            ce.boundary_bands_ragged(st.bits, spec, out=out)
            torch.cuda.synchronize(dev)
            t1 = time.perf_counter()
            each = [boundary_planes(b, H, W, int(d)) for b, (_, H, W), d in zip(bits, chunk, spec[:, 4])]
            torch.cuda.synchronize(dev)
            t2 = time.perf_counter()
            if rep >= 0:
                ragged[rep] += t1 - t0
                per_image[rep] += t2 - t1
            else:
                equal = equal and bool(torch.equal(torch.cat([e.reshape(-1) for e in each]), out))
        chunks += 1
        planes += sum(len(b) for b in bits)
        words_total += st.words

    chunk, words = [], 0
    for iid in gt.img_ids:
        im = gt.image(iid)
        segs = [results[n]["segmentation"] for n in by_img.get(iid, [])] + [g.segmentation for g in gt.gts(iid)]
        if not segs:
            continue
        w = 2 * len(segs) * ((im["height"] * im["width"] + 31) // 32)         # as evaluate_coco counts them for "boundary"
        if chunk and (words + w > ce.CHUNK_WORDS or len(chunk) >= ce.CHUNK_IMAGES):
            run(chunk)
            chunk, words = [], 0
        chunk.append((segs, im["height"], im["width"]))
        words += w
    if chunk:
        run(chunk)
    slower = min(ragged) > max(per_image)
    return {"chunks": chunks, "planes": planes, "plane_words": words_total, "outputs_bitwise_equal": equal,
            "ragged_call_per_chunk_s": _spread(ragged), "boundary_planes_per_image_s": _spread(per_image),
            "ragged_slower_beyond_spread": bool(slower), "ragged_faster_beyond_spread": bool(max(ragged) < min(per_image))}


def measure(n_images, n_small, repeats):
    import torch
    from s2d_amd.coco_eval import evaluate_coco

    def log(msg):
        print(f"[{time.perf_counter() - t_start:7.1f} s] {msg}", file=sys.stderr, flush=True)

    t_start = time.perf_counter()
    dev = torch.device("cuda", 0)
    gen = _generator()
    res = {"device": torch.cuda.get_device_name(0), "repeats": repeats, "dilation_ratio": 0.02}
    for name, n, sizes, dets in (("coco_val_shaped", n_images, gen.SIZES, gen.DETS), ("many_small_images", n_small, SMALL_SIZES, SMALL_DETS)):
        gen.SIZES, gen.DETS = sizes, dets                                      # the generator reads its module's own tables
        t0 = time.perf_counter()
        doc, results = gen.make_set(n, dev, log)
        entry = {"set": {"images": n, "detections": len(results), "ground_truths": len(doc["annotations"]), "sizes": sizes,
                         "detections_per_image": dets, "generate_s": round(time.perf_counter() - t0, 1)}}
        nw = min(50, n)
        warm = ({"images": doc["images"][:nw], "categories": doc["categories"], "annotations": [a for a in doc["annotations"] if a["image_id"] <= nw]},
                [r for r in results if r["image_id"] <= nw])
        for t in ("segm", "boundary"):
            evaluate_coco(*warm, iou_type=t, device=dev)
        runs = {"segm": [], "boundary": []}
        for rep in range(repeats):
            for t in ("segm", "boundary"):
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                ev = evaluate_coco(doc, results, iou_type=t, device=dev, profile=True)
                total = time.perf_counter() - t0
                stats = ev.summarize(out=None)
                runs[t].append({"total_s": total, "seconds": {k: ev.seconds.get(k, 0.0) for k in PHASES}, "library_calls": dict(ev.launches),
                                "AP": round(float(stats[0]), 6), "AR100": round(float(stats[8]), 6)})
                log(f"{name} {t} #{rep}: {total:.3f} s")
        for t, rs in runs.items():
            entry[t] = {"total_s": _spread([r["total_s"] for r in rs]),
                        "seconds": {k: _spread([r["seconds"][k] for r in rs]) for k in PHASES if t == "boundary" or k != "boundary"},
                        "library_calls": rs[-1]["library_calls"], "AP": rs[-1]["AP"], "AR100": rs[-1]["AR100"]}
        entry["band_phase_alone"] = band_phase(doc, results, dev, repeats)
        log(f"{name} band phase: {entry['band_phase_alone']}")
        res[name] = entry
        del doc, results
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=5000)
    ap.add_argument("--small-images", type=int, default=20000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--limit", type=int, default=1100, help="seconds for the measuring child process")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        print(json.dumps(measure(a.images, a.small_images, a.repeats)), flush=True)
        return 0
    t0 = time.perf_counter()
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--images", str(a.images), "--small-images",
                            str(a.small_images), "--repeats", str(a.repeats)], stdout=subprocess.PIPE, text=True, timeout=a.limit, cwd=ROOT)
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
