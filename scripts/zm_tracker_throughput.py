#!/usr/bin/env python3
"""Throughput of the zero-mean block tracker (s2d_amd/keymask/block_tracker.py ZeroMeanBlockTracker) beside the live-template
tracker it shares its search with:

  * ms_per_call: one tracker call at 480 x 854, T = 80, grid 50 on a full-frame mask (2,500 points; query frame 0 forward
    only, and query frame 40 with backward tracking) for search in (16, 32, 64), refresh in (-1, 4) and texture in (0, 4), grey
    frames cached.  Per configuration: warm-up calls, then `repeats` timed loops of `iters` calls, each between two device
    synchronises; the figure is the median of the repeats.  `live_search*_refresh*` is LiveBlockTracker (s2d_block_track_live_u8)
    timed the same way in the same run: the yardstick.  `ratios` is the figure of merit: zero-mean over live at equal search and
    refresh.
  * two textures, the data of scripts/live_tracker_throughput.py: `drift`, a textured frame moving by (1, 3) px per frame, where
    every point finds a zero-cost match, and `noise`, independent random frames, where nothing matches, every point is
    invisible and the cost bound tau (2R+1)^2 ends most candidates after a few rows.  No point of either is untextured, so
    texture 4 gates nothing here: it times the gate's test, not a video with flat regions.
  * driver_ms_per_video: `s2d_amd.keymask.discover.run --tracker block-zm` on the lit scenes of tests/zm_tracker_ref.py (10 / 9
    frames of 120 x 216), tracker included.

    python scripts/zm_tracker_throughput.py [--iters 10] [--repeats 5] [--out profiles/zm_tracker/throughput.json]

Prints one JSON line (progress goes to stderr)."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import zm_tracker_ref as Z  # noqa: E402
from tests.golden import keymask_stub_tracker as S  # noqa: E402

T, H, W = 80, 480, 854
SEARCHES, REFRESHES, TEXTURES = (16, 32, 64), (-1, 4), (0, 4)
CALLS = (("q0_forward", 0, False), ("q40_backward", 40, True))


def _videos():
    rng = np.random.default_rng(0)
    big = np.repeat(np.repeat(rng.integers(0, 256, ((H + T) // 2 + 1, (W + 3 * T) // 2 + 1, 3), dtype=np.uint8), 2, 0), 2, 1)
    drift = np.stack([big[T - t:T - t + H, 3 * (T - t):3 * (T - t) + W] for t in range(T)])
    noise = rng.integers(0, 256, (T, H, W, 3), dtype=np.uint8)
    return {name: torch.from_numpy(f).cuda().permute(0, 3, 1, 2)[None].float().contiguous() for name, f in (("drift", drift), ("noise", noise))}


def _median_ms(tracker, video, mask, q, back, iters, repeats):
    call = lambda: tracker(video, grid_size=50, grid_query_frame=q, segm_mask=mask, backward_tracking=back)
    for _ in range(2):
        tracks, vis = call()
    times = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(iters):
            call()
        torch.cuda.synchronize()
        times.append(1e3 * (time.perf_counter() - t0) / iters)
    return round(statistics.median(times), 3), round(float(vis.float().mean()), 4), int(tracks.shape[2])


def call_ms(iters, repeats):
    from s2d_amd.keymask.block_tracker import LiveBlockTracker, ZeroMeanBlockTracker
    mask = torch.full((1, 1, H, W), 255, dtype=torch.uint8)
    out = {}
    for texture, video in _videos().items():
        res = out[texture] = {}
        for label, q, back in CALLS:
            r = res[label] = {"ratios": {}}
            for s in SEARCHES:
                for u in REFRESHES:
                    live = f"live_search{s}_refresh{u}"
                    r[live], r[live + "_visible_fraction"], r["points"] = _median_ms(LiveBlockTracker(search=s, refresh=u), video, mask, q, back, iters, repeats)
                    for x in TEXTURES:
                        key = f"zm_search{s}_refresh{u}_texture{x}"
                        r[key], r[key + "_visible_fraction"], r[key + "_points"] = _median_ms(
                            ZeroMeanBlockTracker(search=s, refresh=u, texture=x), video, mask, q, back, iters, repeats)
                        r["ratios"][key + "_to_live"] = round(r[key] / r[live], 2)
                        print(f"{texture} {label} {key}: {r[key]} ms, live {r[live]} ms", file=sys.stderr, flush=True)
    return out


def driver_ms():
    from s2d_amd.keymask.discover import parse_args, run
    work = tempfile.mkdtemp(prefix="zmbench")
    cwd = os.getcwd()
    os.chdir(work)
    try:
        Z.write_dataset(".", lit=True)
        args = parse_args(["--video-base-path", S.FRAMES_DIR, "--mask-base-path", S.MASKS_DIR, "--save-path", "seg",
                           "--visibility-maps-output-base", "vmaps", "--visibility-clusters-output-base", "vclusters",
                           "--annotation-output-path", "ann", "--tracker", "block-zm"])
        rep = run(args)
    finally:
        os.chdir(cwd)
    n = max(rep["done"] + rep["failed"], 1)
    return rep, 1e3 * rep["wall_s"] / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from s2d_amd.keymask.block_tracker import ZeroMeanBlockTracker
    d = ZeroMeanBlockTracker()
    t0 = time.perf_counter()
    calls = call_ms(a.iters, a.repeats)
    rep, ms = driver_ms()
    res = {"device": torch.cuda.get_device_name(0), "shape": [T, H, W], "grid": 50, "radius": d.radius, "tau": d.tau,
           "defaults": {"search": d.search, "refresh": d.refresh, "texture": d.texture}, "iters": a.iters, "repeats": a.repeats,
           "ms_per_call": calls, "driver_scenes": sorted(S.SCENES), "driver_report": rep, "driver_ms_per_video_incl_tracker": round(ms, 1),
           "script_s": round(time.perf_counter() - t0, 1)}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
