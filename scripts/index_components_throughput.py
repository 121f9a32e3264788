#!/usr/bin/env python3
"""Throughput of the connected-component cleanup (ops.index_components / ops.filter_components, csrc/index_components.hip), in one
run on an MI355X:

  (a) label + filter against the host: one frame of 720 x 1280 and 70 frames of 480 x 854, for three kinds of content -- `blobs`
      (about 20 elliptic instances and 1 % of the pixels as speckles of a random id), `full` (one id everywhere: one component per
      frame) and `checker4` (a 4-connected checkerboard of one id: every set pixel its own component).  Device: `filter_components`
      (label + filter, min_area 16, keep_largest) and `index_components` alone, each timing `--calls` back-to-back calls between two
      device events divided by the count, median of `repeats` after a warm-up.  Host: what a user has without the op --
      scipy.ndimage.label per id over the same maps, the areas by bincount and the same keep rule -- wall time, median of `repeats`.
      The two outputs are checked equal.
  (b) whole driver: frame_masks.write_masks on the synthetic tree of scripts/frame_masks_throughput.py (30 sequences x `--frames`
      frames of 480 x 854), the same seeded model, --frames-per-call 1 and 8, with the cleanup off and on (min area 16, keep largest):
      frames/s, median of `repeats` runs after a warm-up run.  `parent` repeats the option-off figures and runs recorded in
      profiles/frame_masks/throughput.json for comparison.
  (c) `--kernels-only`: a few calls of (a)'s device side and nothing else, the program to put behind
      `rocprofv3 --kernel-trace --stats --` for the per-launch breakdown (a run of its own); `--kernel-stats FILE` folds that run's
      kernel_stats CSV into the JSON as `per_launch`.

    python scripts/index_components_throughput.py [--repeats 3] [--frames 24] [--out profiles/index_components/throughput.json]

The measurement runs in a child process under a time limit; prints one JSON line.  Without a GPU it fails."""
import argparse
import csv
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(1, HERE)

SHAPES = {"1x720x1280": (1, 720, 1280), "70x480x854": (70, 480, 854)}
MIN_AREA = 16
KERNELS = ("cc_tile_kernel", "cc_merge_kernel", "cc_flatten_kernel", "cc_best_kernel", "cc_filter_kernel", "zero_kernel")


def content(kind, N, H, W):
    """-> (index u8 [N,H,W], connectivity)"""
    import numpy as np
    if kind == "full":
        return np.full((N, H, W), 1, np.uint8), 8
    yy, xx = np.mgrid[0:H, 0:W]
    if kind == "checker4":
        return np.broadcast_to(((yy + xx) % 2 == 0).astype(np.uint8), (N, H, W)).copy(), 4
    rng = np.random.default_rng(H + N)
    base = np.zeros((H, W), np.uint8)
    for k in range(20):
        cy, cx, ry, rx = rng.uniform(0, H), rng.uniform(0, W), rng.uniform(H / 16, H / 5), rng.uniform(W / 16, W / 5)
        base[((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 < 1.0] = k + 1
    out = np.empty((N, H, W), np.uint8)
    for n in range(N):
        frame = np.roll(base, 5 * n, axis=1)
        noise = rng.random((H, W)) < 0.01
        frame[noise] = rng.integers(1, 21, int(noise.sum()), dtype=np.uint8)
        out[n] = frame
    return out, 8


def host_filter(index, min_area, keep_largest, conn):
    """the host path: scipy.ndimage.label per id, areas by bincount, the op's keep rule (equal areas: the lower first pixel, which is
    the lower scipy label -- scipy numbers components in raster order of their first pixels)"""
    import numpy as np
    from scipy import ndimage
    st = ndimage.generate_binary_structure(2, 1 if conn == 4 else 2)
    out = np.zeros_like(index)
    for n in range(index.shape[0]):
        for v in np.unique(index[n]):
            if v == 0:
                continue
            lab, k = ndimage.label(index[n] == v, st)
            area = np.bincount(lab.reshape(-1), minlength=k + 1)
            area[0] = 0
            keep = area >= max(min_area, 1)
            if keep_largest:
                best = int(np.argmax(area))                               # the first of the largest
                keep &= np.arange(k + 1) == best
            out[n][keep[lab]] = v
    return out


def _host_ms(fn, repeats):
    ms = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ms)


def label_phase(repeats, calls, kinds=("blobs", "full", "checker4")):
    import numpy as np
    import torch
    from frame_masks_throughput import _timed
    from s2d_amd import ops
    res = {"min_area": MIN_AREA, "keep_largest": True, "tile": list(ops.component_tile())}
    for shape_name, (N, H, W) in SHAPES.items():
        for kind in kinds:
            index, conn = content(kind, N, H, W)
            dev = torch.from_numpy(index).to("cuda:0")
            out, removed = ops.filter_components(dev, MIN_AREA, True, conn)
            _, area = ops.index_components(dev, conn)
            row = {"connectivity": conn, "components": int((area > 0).sum()), "removed_pixels": int(removed.sum())}
            del area
            want = host_filter(index, MIN_AREA, True, conn)
            row["equal_to_host"] = bool(np.array_equal(out.cpu().numpy(), want))
            del out, want
            row["label_filter_ms"] = round(_timed(lambda: ops.filter_components(dev, MIN_AREA, True, conn), repeats, calls)[0], 4)
            row["label_ms"] = round(_timed(lambda: ops.index_components(dev, conn), repeats, calls)[0], 4)
            row["host_scipy_ms"] = round(_host_ms(lambda: host_filter(index, MIN_AREA, True, conn), repeats), 1)
            row["host_over_device"] = round(row["host_scipy_ms"] / row["label_filter_ms"], 1)
            res[f"{shape_name}_{kind}"] = row
            print(f"label phase {shape_name} {kind}: {row}", file=sys.stderr, flush=True)
            del dev
    return res


def driver_phase(frames, repeats):
    import torch
    from frame_masks_throughput import SEQS, H, W, _write_tree
    from s2d_amd.config import load_config
    from s2d_amd.keymask.frame_masks import write_masks
    from s2d_amd.modeling.meta_arch import META_ARCH_REGISTRY
    cfg = load_config(os.path.join(ROOT, "tests", "golden", "kd_config.json"), ["MODEL.MASK_FORMER.TEST.NUM_PREDICTIONS", "50"])
    torch.manual_seed(0)
    model = META_ARCH_REGISTRY.get(cfg.MODEL.META_ARCHITECTURE).from_config(cfg).to("cuda:0")
    res = {"sequences": SEQS, "frames_per_sequence": frames, "size": [H, W], "threads": 16, "min_area": MIN_AREA, "keep_largest": True}
    parent = os.path.join(ROOT, "profiles", "frame_masks", "throughput.json")
    recorded = json.load(open(parent))["driver"] if os.path.isfile(parent) else {}
    with tempfile.TemporaryDirectory() as root:
        img_root = _write_tree(root, frames)
        for per_call in (1, 8):
            row = {}
            for name, extra in (("off", {}), ("on", {"min_component_area": MIN_AREA, "keep_largest": True})):
                lines = []
                for i in range(repeats + 1):                            # the first run is the warm-up
                    lines.append(write_masks(cfg, model, img_root, os.path.join(root, f"masks_{per_call}_{name}_{i}"), 0.0, 50, per_call,
                                             threads=16, **extra))
                    print(f"driver run {i}, cleanup {name}, {per_call} frames per call: {lines[-1]}", file=sys.stderr, flush=True)
                timed = lines[1:]
                row[name] = {"frames": timed[0]["frames"], "removed_pixels": timed[0]["removed_pixels"],
                             "frames_per_s": round(statistics.median(l["frames_per_s"] for l in timed), 1),
                             "runs_frames_per_s": [l["frames_per_s"] for l in timed]}
            rec = recorded.get(f"frames_per_call_{per_call}")
            if rec:
                row["parent"] = {"frames_per_s": rec["frames_per_s"], "runs_frames_per_s": [r["frames_per_s"] for r in rec["runs"]]}
            res[f"frames_per_call_{per_call}"] = row
    return res


def kernels_only():
    """(c): a few calls per shape and content, nothing timed here"""
    import torch
    from s2d_amd import ops
    for N, H, W in SHAPES.values():
        for kind in ("blobs", "full", "checker4"):
            index, conn = content(kind, N, H, W)
            dev = torch.from_numpy(index).to("cuda:0")
            for _ in range(5):
                ops.filter_components(dev, MIN_AREA, True, conn)
            torch.cuda.synchronize()
    print(json.dumps({"kernels_only": True, "calls_per_case": 5, "cases": 6}), flush=True)


def per_launch(path):
    """rocprofv3's kernel_stats CSV -> {kernel: {calls, total_us, mean_us, percent}} for this feature's kernels"""
    rows = {}
    with open(path) as fh:
        for r in csv.DictReader(fh):
            name = r["Name"]
            key = next((k for k in KERNELS if k in name), None)
            if key:
                rows[key] = {"calls": int(r["Calls"]), "total_us": round(float(r["TotalDurationNs"]) / 1e3, 1),
                             "mean_us": round(float(r["AverageNs"]) / 1e3, 2), "percent": round(float(r["Percentage"]), 2)}
    return rows


def measure(repeats, frames, calls):
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this script measures on an MI355X only")
    return {"device": torch.cuda.get_device_name(0), "repeats": repeats, "calls_per_timing": calls,
            "label_filter": label_phase(repeats, calls), "driver": driver_phase(frames, repeats)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--frames", type=int, default=24, help="frames per sequence of the synthetic tree")
    ap.add_argument("--calls", type=int, default=20, help="back-to-back calls per kernel timing")
    ap.add_argument("--limit", type=int, default=1100, help="seconds for the measuring child process")
    ap.add_argument("--out", default=None)
    ap.add_argument("--kernel-stats", default=None, help="kernel_stats CSV of a rocprofv3 run of --kernels-only, folded in as per_launch")
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.repeats < 3:
        ap.error("medians of at least 3")
    if a.kernels_only:
        kernels_only()
        return 0
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
    if a.kernel_stats:
        res["per_launch"] = per_launch(a.kernel_stats)
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
