#!/usr/bin/env python3
"""Throughput of the stage-1 frame-mask driver (`python -m s2d_amd.keymask.frame_masks`), in one run on an MI355X:

  (a) paint phase at DAVIS 480p: output 480 x 854 from logits of a 360-pixel test size (maps 90 x 160, input 360 x 640, no padding,
      Q = 100 columns), K = 20 and 50 proposals, T = 1 and 8 frames.  `ops.paint_frames` (plane-free areas + order + paint) against
      the composition available without it: `ops.infer_masks` (the [K,T,oh,ow] byte planes) -> `ops.mask_frame_areas` ->
      `ops.render_instances(zeros, ..., alpha=256)`.  The two alternate within one process; each timing is `--calls` back-to-back
      calls between two device events, divided by the count; median of `repeats` after a warm-up; the peak of
      torch.cuda.max_memory_allocated above the resident inputs over one call; the two pictures are checked equal.
  (b) whole driver: frame_masks.write_masks on a synthetic tree of 30 sequences x `--frames` frames of 480 x 854 JPEGs, a seeded model
      (tests/golden/kd_config.json, random weights, 50 predictions, threshold 0), --frames-per-call 1 and 8: frames/s, the
      loader-wait fraction, and the seconds inside PNG encoding (summed over the pool's threads) over wall time -- a figure above 1
      means more than one thread's worth; median of `repeats` runs after a warm-up run.

    python scripts/frame_masks_throughput.py [--repeats 3] [--frames 24] [--limit 1100] [--out profiles/frame_masks/throughput.json]

The measurement runs in a child process under a time limit; prints one JSON line.  Without a GPU it fails."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H, W, Q = 480, 854, 100
PADDED, IMG, HM, WM = (360, 640), (360, 640), 90, 160
SEQS = 30


def _timed(fn, repeats, calls):
    """-> (median ms per call by device events over `calls` back-to-back calls, peak bytes of one call above what was allocated)"""
    import torch
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1) / calls)
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return statistics.median(ms), peak


def paint_phase(K, T, repeats, calls):
    import torch
    from s2d_amd import ops
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(K * 100 + T)
    coarse = torch.randn((Q * T, 1, 6, 6), device=dev, generator=g) * 3.0
    planes = torch.nn.functional.interpolate(coarse, size=(HM, WM), mode="bicubic", align_corners=True)[:, 0]
    ml = planes.view(Q, T * HM * WM).t().contiguous()
    query = torch.randperm(Q, device=dev, generator=g)[:K].to(torch.int32).contiguous()
    colors = torch.from_numpy(ops.mask_colors(K)).to(dev)
    del coarse, planes
    dims, out = (T, HM, WM), (H, W)
    zeros = torch.zeros((T, H, W, 3), device=dev, dtype=torch.uint8)

    def new():
        return ops.paint_frames(ml, dims, PADDED, IMG, out, query, colors)

    def composed():
        masks, _ = ops.infer_masks(ml, dims, PADDED, IMG, out, query)
        areas, order = ops.mask_frame_areas(masks)
        return ops.render_instances(zeros, masks, order, colors, alpha=256, want_index=False)[0], areas, order

    rgb, _, areas, order = new()
    rgb_c, areas_c, order_c = composed()
    res = {"pictures_equal": bool(torch.equal(rgb, rgb_c) and torch.equal(areas, areas_c) and torch.equal(order, order_c)),
           "painted_share": round(float((rgb != 0).any(-1).float().mean()), 4)}
    del rgb, rgb_c, areas, areas_c, order, order_c
    rows = {"paint_frames": [], "infer_masks_areas_render": []}
    peaks = {}
    for _ in range(2):                                                   # the two alternate; the medians of both rounds are kept
        for name, fn in (("paint_frames", new), ("infer_masks_areas_render", composed)):
            ms, peak = _timed(fn, repeats, calls)
            rows[name].append(ms)
            peaks[name] = int(peak)
    for name in rows:
        res[name] = {"ms": round(statistics.median(rows[name]), 4), "ms_rounds": [round(v, 4) for v in rows[name]], "peak_bytes": peaks[name]}
    ms, _ = _timed(lambda: ops.infer_frame_areas(ml, dims, PADDED, IMG, out, query), repeats, calls)
    res["infer_frame_areas_alone_ms"] = round(ms, 4)
    _, order = ops.infer_frame_areas(ml, dims, PADDED, IMG, out, query)
    ms, _ = _timed(lambda: ops.infer_paint(ml, dims, PADDED, IMG, out, query, order, colors), repeats, calls)
    res["infer_paint_alone_ms"] = round(ms, 4)
    res["planes_bytes"] = K * T * H * W
    return res


def _write_tree(root, frames):
    import numpy as np
    from PIL import Image
    rng = np.random.default_rng(0)
    img_root = os.path.join(root, "DAVIS", "JPEGImages", "480p")
    base = rng.integers(0, 255, (H, W, 3), dtype=np.uint8)
    for s in range(SEQS):
        name = f"seq{s:02d}"
        os.makedirs(os.path.join(img_root, name))
        for t in range(frames):
            Image.fromarray(np.roll(base, (s * 7 + t * 3) % W, axis=1)).save(os.path.join(img_root, name, f"{t:05d}.jpg"), quality=85)
    return img_root


def driver_phase(frames, repeats):
    import torch
    from s2d_amd.config import load_config
    from s2d_amd.keymask.frame_masks import write_masks
    from s2d_amd.modeling.meta_arch import META_ARCH_REGISTRY
    cfg = load_config(os.path.join(ROOT, "tests", "golden", "kd_config.json"), ["MODEL.MASK_FORMER.TEST.NUM_PREDICTIONS", "50"])
    torch.manual_seed(0)
    model = META_ARCH_REGISTRY.get(cfg.MODEL.META_ARCHITECTURE).from_config(cfg).to("cuda:0")
    res = {"sequences": SEQS, "frames_per_sequence": frames, "size": [H, W], "threads": 16}
    with tempfile.TemporaryDirectory() as root:
        t0 = time.perf_counter()
        img_root = _write_tree(root, frames)
        res["tree_write_s"] = round(time.perf_counter() - t0, 1)
        for per_call in (1, 8):
            lines = []
            for i in range(repeats + 1):                                # the first run is the warm-up
                lines.append(write_masks(cfg, model, img_root, os.path.join(root, f"masks_{per_call}_{i}"), 0.0, 50, per_call, threads=16))
                print(f"driver run {i} at {per_call} frames per call: {lines[-1]}", file=sys.stderr, flush=True)
            timed = lines[1:]
            res[f"frames_per_call_{per_call}"] = {
                "frames": timed[0]["frames"], "masks": timed[0]["masks"], "empty_frames": timed[0]["empty_frames"],
                "frames_per_s": round(statistics.median(l["frames_per_s"] for l in timed), 1),
                "wall_s": round(statistics.median(l["wall_s"] for l in timed), 2),
                "loader_wait_fraction": round(statistics.median(l["loader_wait_fraction"] for l in timed), 4),
                "encode_s_over_wall_s": round(statistics.median(l["encode_s"] / l["wall_s"] for l in timed), 4),
                "runs": [{k: l[k] for k in ("frames_per_s", "wall_s", "loader_wait_fraction", "encode_s")} for l in timed]}
    return res


def measure(repeats, frames, calls):
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this script measures on an MI355X only")
    res = {"device": torch.cuda.get_device_name(0), "repeats": repeats, "calls_per_timing": calls,
           "paint_phase": {"output": [H, W], "maps": [HM, WM], "padded": list(PADDED), "image": list(IMG), "ldq": Q}}
    for K in (20, 50):
        for T in (1, 8):
            res["paint_phase"][f"K{K}_T{T}"] = paint_phase(K, T, repeats, calls)
            print(f"paint phase K = {K}, T = {T} done", file=sys.stderr, flush=True)
    res["driver"] = driver_phase(frames, repeats)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--frames", type=int, default=24, help="frames per sequence of the synthetic tree")
    ap.add_argument("--calls", type=int, default=50, help="back-to-back calls per kernel timing")
    ap.add_argument("--limit", type=int, default=1100, help="seconds for the measuring child process")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.repeats < 3:
        ap.error("medians of at least 3")
    if a.child:
        print(json.dumps(measure(a.repeats, a.frames, a.calls)), flush=True)
        return 0
    t0 = time.perf_counter()
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--repeats", str(a.repeats), "--frames", str(a.frames),
                            "--calls", str(a.calls)], stdout=subprocess.PIPE, text=True, timeout=a.limit, cwd=ROOT)   # progress: stderr
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
