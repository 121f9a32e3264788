#!/usr/bin/env python3
"""Keymask discovery throughput at the BASELINE config-3 shape (32 frames of 480 x 854, 6 objects per frame) with the
deterministic stub tracker of tests/golden/keymask_stub_tracker.py:

  * driver_ms_per_video: wall time of `s2d_amd.keymask.discover.run` per video minus the time spent inside tracker calls;
  * us_per_tracked_mask: one tracked mask's (frame, object) counts (2,500 points per frame, the grid-50 upper bound) by
    s2d_track_point_id_counts against s2d_tracks_to_masks_u8 + s2d_point_id_counts, device time by events.

    python scripts/keymask_throughput.py [--videos 2] [--iters 200] [--out FILE]

Prints one JSON line."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests.golden import keymask_stub_tracker as S  # noqa: E402

T, H, W = 32, 480, 854


def scene():
    objs = []
    for i in range(6):
        y, x = 30 + 70 * i, 20 + 110 * i
        objs.append(dict(color=(40 * i + 20, 255 - 35 * i, 90 + 25 * i), shade=(200 - 30 * i, 60 + 30 * i, 120),
                         box=(min(y, H - 120), x, 110, 150), step=((-1) ** i, 3 + i), absent=(range(10, 14) if i == 5 else ())))
    return dict(T=T, H=H, W=W, objects=objs)


def driver_ms(videos):
    from s2d_amd.keymask.discover import parse_args, run
    sc = scene()
    work = tempfile.mkdtemp(prefix="kmbench")
    cwd = os.getcwd()
    os.chdir(work)
    try:
        S.write_dataset(".", {f"v{i:02d}": sc for i in range(videos)})
        args = parse_args(["--video-base-path", S.FRAMES_DIR, "--mask-base-path", S.MASKS_DIR, "--save-path", "seg",
                           "--visibility-maps-output-base", "vmaps", "--visibility-clusters-output-base", "vclusters",
                           "--annotation-output-path", "ann"])
        tracker = S.StubTracker({f"v{i:02d}": sc for i in range(videos)})
        rep = run(args, tracker=tracker)
    finally:
        os.chdir(cwd)
    n = max(rep["done"] + rep["failed"], 1)
    return rep, len(tracker.calls), 1e3 * (rep["wall_s"] - rep["tracker_s"]) / n


def kernel_us(iters):
    from s2d_amd.keymask import IdMap, point_id_counts, point_id_counts_from_tracks, pred_tracks_to_binary_masks
    rng = np.random.default_rng(0)
    ids = np.zeros((T, H, W), np.int64)
    for o in range(6):
        ids[:, 60 * o:60 * o + 120, 100 * o:100 * o + 200] = o + 1
    idmap = IdMap(torch.from_numpy(ids))
    tracks = torch.from_numpy(np.stack([rng.uniform(0, W, (T, 2500)), rng.uniform(0, H, (T, 2500))], -1).astype(np.float32)).cuda()[None]

    def fused():
        return point_id_counts_from_tracks(tracks, H, W, idmap)

    def two():
        return point_id_counts(pred_tracks_to_binary_masks(tracks, H, W)[0], idmap)

    a, b = fused(), two()
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    out = {}
    for name, fn in (("fused", fused), ("two_launch", two)):
        for _ in range(20):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out[name] = 1e3 * e0.elapsed_time(e1) / iters
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--videos", type=int, default=2)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    t0 = time.perf_counter()
    rep, calls, ms = driver_ms(a.videos)
    us = kernel_us(a.iters)
    res = {"device": torch.cuda.get_device_name(0), "shape": [T, H, W], "objects": 6, "videos": a.videos, "report": rep,
           "tracker_calls": calls, "driver_ms_per_video_excl_tracker": round(ms, 1),
           "us_per_tracked_mask": {k: round(v, 1) for k, v in us.items()}, "script_s": round(time.perf_counter() - t0, 1)}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
