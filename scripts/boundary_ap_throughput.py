#!/usr/bin/env python3
"""Throughput of Boundary AP (csrc/mask_boundary.hip, s2d_amd/ytvis_eval.py) on one video of 36 frames at 720 x 1280 with 10 and
50 tracks (as many detections as ground truths, moving discs), in one run:

  * kernel: s2d_mask_boundary_bits_u32 on the video's detection planes (tracks x 36 planes, d = 29), ms by device events and
    algorithmic GB/s (one plane read plus one written per plane);
  * evaluate_ytvis on the video's RLE results, wall ms per video to the returned YTVISEval, with iou_type "segm" and "boundary",
    and their ratio: what Boundary AP costs beside mask AP for the same video.

    python scripts/boundary_ap_throughput.py [--iters 20] [--limit 300] [--out profiles/boundary_ap/throughput.json]

The measurement runs in a child process under a time limit; prints one JSON line."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

T, H, W = 36, 720, 1280
TRACKS = (10, 50)


def disc_tracks(K, seed, dev):
    """K tracks of T frames: one disc each, drifting, some cut by the image edge -> CUDA u8 [K, T, H, W]"""
    import torch
    g = torch.Generator().manual_seed(seed)
    cy = (torch.rand(K, generator=g) * H).to(dev)
    cx = (torch.rand(K, generator=g) * W).to(dev)
    r = (40 + torch.rand(K, generator=g) * 260).to(dev)
    v = ((torch.rand(K, 2, generator=g) - 0.5) * 6).to(dev)
    t = torch.arange(T, device=dev, dtype=torch.float32)[:, None, None]
    yy = torch.arange(H, device=dev, dtype=torch.float32)[None, :, None]
    xx = torch.arange(W, device=dev, dtype=torch.float32)[None, None, :]
    out = torch.empty((K, T, H, W), device=dev, dtype=torch.uint8)
    for k in range(K):
        out[k] = ((yy - (cy[k] + v[k, 0] * t)) ** 2 + (xx - (cx[k] + v[k, 1] * t)) ** 2) < r[k] * r[k]
    return out


def measure(iters):
    import torch
    from s2d_amd import ops
    from s2d_amd.rle import encode_video_predictions
    from s2d_amd.ytvis_eval import boundary_dilation, boundary_planes, evaluate_ytvis
    dev = torch.device("cuda", 0)
    d = boundary_dilation(H, W)
    res = {"device": torch.cuda.get_device_name(0), "shape": [T, H, W], "dilation": d, "iters": iters, "tracks": {}}
    for K in TRACKS:
        gt_m, dt_m = disc_tracks(K, K, dev), disc_tracks(K, K, dev).roll(3, dims=3)
        bits = ops.pack_mask_bits(dt_m.view(K * T, H * W))
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for timed in (False, True):
            torch.cuda.synchronize()
            e0.record()
            for _ in range(iters if timed else 3):
                band = boundary_planes(bits, H, W, d)
            e1.record()
            torch.cuda.synchronize()
        k_ms = e0.elapsed_time(e1) / iters
        nbytes = 2 * bits.numel() * 4
        doc = {"videos": [{"id": 1, "height": H, "width": W, "length": T}], "categories": [{"id": 1, "name": "object"}],
               "annotations": [{"id": 1 + k, "video_id": 1, "category_id": 1, "iscrowd": 0, "segmentations": s,
                                "areas": [int(a) for a in gt_m[k].sum((1, 2)).tolist()]} for k, s in enumerate(encode_video_predictions(gt_m))]}
        results = [{"video_id": 1, "score": 1.0 - 0.01 * k, "category_id": 1, "segmentations": s}
                   for k, s in enumerate(encode_video_predictions(dt_m))]
        ev_ms, stats = {}, {}
        for kind in ("segm", "boundary"):
            for timed in (False, True):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(max(iters // 4, 3) if timed else 1):
                    ev = evaluate_ytvis(doc, results, iou_type=kind)
                torch.cuda.synchronize()
                ev_ms[kind] = 1e3 * (time.perf_counter() - t0) / max(iters // 4, 3)
            stats[kind] = round(float(ev.summarize(out=None)[0]), 4)
        res["tracks"][str(K)] = {"planes": K * T, "kernel_ms": round(k_ms, 4), "kernel_GBps": round(nbytes / (k_ms * 1e-3) / 1e9, 1),
                                 "band_fraction_of_mask": round(_popcount(band) / max(_popcount(bits), 1), 4),
                                 "evaluate_ytvis_ms_per_video": {k: round(v, 2) for k, v in ev_ms.items()},
                                 "boundary_over_segm": round(ev_ms["boundary"] / ev_ms["segm"], 3), "AP": stats}
        del gt_m, dt_m, bits, band
    return res


def _popcount(bits):
    from s2d_amd.ytvis_eval import plane_areas
    return int(plane_areas(bits).to("cpu").sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--limit", type=int, default=300, help="seconds for the measuring child process")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        print(json.dumps(measure(a.iters)), flush=True)
        return 0
    t0 = time.perf_counter()
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--iters", str(a.iters)], capture_output=True, text=True,
                           timeout=a.limit, cwd=ROOT)
    except subprocess.TimeoutExpired:
        print(f"the measurement exceeded {a.limit} s", file=sys.stderr)
        return 1
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    if r.returncode != 0 or not lines:
        print(f"the measurement failed with status {r.returncode}:\n{r.stderr[-3000:]}", file=sys.stderr)
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
