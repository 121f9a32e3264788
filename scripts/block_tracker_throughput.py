#!/usr/bin/env python3
"""Throughput of the built-in block tracker (s2d_amd/keymask/block_tracker.py):

  * ms_per_call: one tracker call at 480 x 854, T = 80, grid 50 on a full-frame mask (2,500 points, query frame 0, forward
    only, and query frame 40 with backward tracking), wall time to a device synchronise -- with the grey frames cached (the
    grey pass outside the call, as in discovery after a video's first call) and with the cache dropped before every call
    (the grey pass inside); grey_pass_ms is the pass alone, by device events;
  * driver_ms_per_video: `s2d_amd.keymask.discover.run --tracker block` on the textured scenes of tests/block_tracker_ref.py
    (10 / 9 frames of 120 x 216), tracker included.

    python scripts/block_tracker_throughput.py [--iters 20] [--out profiles/block_tracker/throughput.json]

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

from tests import block_tracker_ref as B  # noqa: E402
from tests.golden import keymask_stub_tracker as S  # noqa: E402

T, H, W = 80, 480, 854


def call_ms(iters):
    from s2d_amd._lib import lib
    from s2d_amd.keymask.block_tracker import BlockTracker
    rng = np.random.default_rng(0)
    # a textured frame drifting by (1, 3) px per frame: every point has something to follow
    big = np.repeat(np.repeat(rng.integers(0, 256, ((H + T) // 2 + 1, (W + 3 * T) // 2 + 1, 3), dtype=np.uint8), 2, 0), 2, 1)
    frames = np.stack([big[T - t:T - t + H, 3 * (T - t):3 * (T - t) + W] for t in range(T)])
    video = torch.from_numpy(frames).cuda().permute(0, 3, 1, 2)[None].float().contiguous()
    mask = torch.full((1, 1, H, W), 255, dtype=torch.uint8)
    tracker = BlockTracker()
    out = {}
    for label, q, back in (("q0_forward", 0, False), ("q40_backward", 40, True)):
        tracks, vis = tracker(video, grid_size=50, grid_query_frame=q, segm_mask=mask, backward_tracking=back)
        for cached in (True, False):
            for timed in (False, True):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(iters if timed else 3):
                    if not cached:
                        tracker._video = None                       # drop the cached grey frames
                    tracker(video, grid_size=50, grid_query_frame=q, segm_mask=mask, backward_tracking=back)
                torch.cuda.synchronize()
                ms = 1e3 * (time.perf_counter() - t0) / iters
            out[f"{label}_{'grey_cached' if cached else 'grey_inside'}"] = round(ms, 3)
        out[f"{label}_visible_fraction"] = round(float(vis.float().mean()), 4)
        out[f"{label}_points"] = int(tracks.shape[2])
    grey = torch.empty((T, H, W), device="cuda", dtype=torch.uint8)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for timed in (False, True):
        torch.cuda.synchronize()
        e0.record()
        for _ in range(iters if timed else 3):
            lib().call("s2d_video_grey_u8", video, T, H, W, grey, torch.cuda.current_stream().cuda_stream)
        e1.record()
        torch.cuda.synchronize()
    out["grey_pass_ms"] = round(e0.elapsed_time(e1) / iters, 3)
    return out


def driver_ms():
    from s2d_amd.keymask.discover import parse_args, run
    work = tempfile.mkdtemp(prefix="btbench")
    cwd = os.getcwd()
    os.chdir(work)
    try:
        B.write_textured_dataset(".")
        args = parse_args(["--video-base-path", S.FRAMES_DIR, "--mask-base-path", S.MASKS_DIR, "--save-path", "seg",
                           "--visibility-maps-output-base", "vmaps", "--visibility-clusters-output-base", "vclusters",
                           "--annotation-output-path", "ann", "--tracker", "block"])
        rep = run(args)
    finally:
        os.chdir(cwd)
    n = max(rep["done"] + rep["failed"], 1)
    return rep, 1e3 * rep["wall_s"] / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    t0 = time.perf_counter()
    calls = call_ms(a.iters)
    rep, ms = driver_ms()
    res = {"device": torch.cuda.get_device_name(0), "shape": [T, H, W], "grid": 50, "radius": B.R, "search": B.SEARCH, "tau": B.TAU,
           "ms_per_call": calls, "driver_scenes": sorted(S.SCENES), "driver_report": rep,
           "driver_ms_per_video_incl_tracker": round(ms, 1), "script_s": round(time.perf_counter() - t0, 1)}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
