#!/usr/bin/env python3
"""Throughput of the eval-only driver (python -m s2d_amd.evaluate) on a seeded synthetic YTVIS-2021-like split.

    python scripts/eval_throughput.py --out DIR [--videos 16] [--frames 36] [--height 720] [--width 1280] [--threads 8] [--rocprof]

Writes the JPEG videos, a GT JSON and a seeded KD checkpoint under DIR, runs the driver on them and prints its timing line
(videos/s and frames/s from a host clock around synchronised work, the fraction of the wall time the model waited on the
loader).  --rocprof adds a SEPARATE run of the driver under `rocprofv3 --kernel-trace --stats` and reports the resize kernel's
time per video and its achieved bytes/s against T*H0*W0*3 + T*3*H1*W1 bytes per video."""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
KD_CFG = os.path.join(ROOT, "tests", "golden", "kd_config.json")


def write_split(root, videos, frames, h, w, seed=0):
    from PIL import Image
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    vids = []
    for v in range(1, videos + 1):
        os.makedirs(os.path.join(root, f"v{v:03d}"), exist_ok=True)
        names = []
        cx, cy = rng.uniform(0.2, 0.8, 2)
        for t in range(frames):
            blob = (((xx / w - cx - 0.005 * t) ** 2 + (yy / h - cy) ** 2) < 0.02)
            img = np.stack([(xx // 4 + 3 * t) % 256, (yy // 3 + 17 * v) % 256, blob * 200 + 20], -1).astype(np.int32)
            img = np.clip(img + rng.integers(-12, 12, img.shape), 0, 255).astype(np.uint8)
            name = f"v{v:03d}/{t:05d}.jpg"
            Image.fromarray(img).save(os.path.join(root, name), quality=90)
            names.append(name)
        vids.append({"id": v, "height": h, "width": w, "length": frames, "file_names": names})
    gt = {"info": {}, "licenses": [], "categories": [{"id": 1, "name": "object"}], "videos": vids}
    path = os.path.join(root, "gt.json")
    with open(path, "w") as fh:
        json.dump(gt, fh)
    return path


def write_checkpoint(path, seed=0):
    import torch
    from s2d_amd.config import load_config
    from s2d_amd.modeling.meta_arch import META_ARCH_REGISTRY
    cfg = load_config(KD_CFG)
    torch.manual_seed(seed)
    model = META_ARCH_REGISTRY.get(cfg.MODEL.META_ARCHITECTURE).from_config(cfg)
    torch.save({"model": model.state_dict()}, path)


def driver_cmd(a, gt, ckpt, out):
    return [sys.executable, "-m", "s2d_amd.evaluate", "--config-file", KD_CFG, "--gt", gt, "--image-root", a.out,
            "--output-dir", out, "--weights", ckpt, "--threads", str(a.threads)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--videos", type=int, default=16)
    ap.add_argument("--frames", type=int, default=36)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--threads", type=int, default=8)
    ap.add_argument("--rocprof", action="store_true")
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    gt = write_split(a.out, a.videos, a.frames, a.height, a.width)
    ckpt = os.path.join(a.out, "ckpt.pth")
    write_checkpoint(ckpt)
    r = subprocess.run(driver_cmd(a, gt, ckpt, os.path.join(a.out, "eval")), capture_output=True, text=True, cwd=ROOT)
    if r.returncode != 0:
        sys.stderr.write(r.stderr[-4000:])
        sys.exit(r.returncode)
    line = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    report = {"videos": a.videos, "frames_per_video": a.frames, "size": [a.height, a.width], "threads": a.threads, "driver": line}
    print(json.dumps(report), flush=True)
    if a.rocprof:
        from s2d_amd.data.augment import shortest_edge_shape
        prof = os.path.join(a.out, "prof")
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", prof, "-o", "run", "--"] + driver_cmd(a, gt, ckpt, os.path.join(a.out, "eval_prof"))
        rp = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT)
        if rp.returncode != 0:
            sys.stderr.write(rp.stderr[-4000:])
            sys.exit(rp.returncode)
        stats = sorted(glob.glob(os.path.join(prof, "**", "*kernel_stats.csv"), recursive=True))
        row = None
        for p in stats:
            for rw in csv.DictReader(open(p)):
                if "resize_bilinear_u8_kernel" in rw["Name"]:
                    row = rw
        if row is None:
            found = [os.path.relpath(p, prof) for p in glob.glob(os.path.join(prof, "**", "*"), recursive=True)]
            raise RuntimeError(f"no resize kernel in {stats} (files: {found[:20]})")
        H1, W1 = shortest_edge_shape(a.height, a.width, 360, 1333)
        calls, total_ns = int(row["Calls"]), float(row["TotalDurationNs"])
        per_video_s = total_ns / calls * 1e-9
        nbytes = a.frames * a.height * a.width * 3 + a.frames * 3 * H1 * W1
        report["resize_kernel"] = {"calls": calls, "us_per_video": round(per_video_s * 1e6, 2), "bytes_per_video": nbytes,
                                   "GB_per_s": round(nbytes / per_video_s / 1e9, 1)}
        print(json.dumps({"resize_kernel": report["resize_kernel"]}), flush=True)


if __name__ == "__main__":
    main()
