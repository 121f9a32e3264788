#!/usr/bin/env python3
"""Throughput of the hole filling of index maps (ops.fill_index_holes, csrc/index_components.hip), in one run on an MI355X:

  (a) label + filter + fill against label + filter alone -- the yardstick of profiles/index_components/throughput.json, re-taken in
      this run -- and against the host.  Inputs: one frame of 720 x 1280 of about 20 blobs with 1 % speckle (`blobs`, the content of
      scripts/index_components_throughput.py), the frame-sized ring of that size (`ring`: ONE hole of (H-2)(W-2) pixels, every
      boundary pixel of which reports to one root) and 70 frames of 480 x 854 of blobs.  Device: `filter_components` (min_area 16,
      keep_largest), then `fill_index_holes` ("all") on its output; each timing is `--calls` back-to-back calls between two device
      events divided by the count, median of `repeats` after a warm-up.  Host: scipy.ndimage.label per frame over the zero pixels and
      a dilation per hole (tests/index_fill_refs.py) -- wall time, median of `repeats`.  The outputs are asserted equal.
  (b) whole driver: frame_masks.write_masks on the synthetic tree of scripts/frame_masks_throughput.py (30 sequences x `--frames`
      frames of 480 x 854), the same seeded model, --frames-per-call 1 and 8, cleanup on (min area 16, keep largest), with
      --fill-holes off and all: frames/s, median of `repeats` runs after a warm-up run.

    python scripts/index_fill_throughput.py [--repeats 3] [--frames 24] [--out profiles/index_fill/throughput.json]

The measurement runs in a child process under a time limit; prints one JSON line.  Without a GPU it fails."""
import argparse
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

MIN_AREA = 16
CASES = {"1x720x1280_blobs": ("blobs", 1, 720, 1280), "1x720x1280_ring": ("ring", 1, 720, 1280),
         "70x480x854_blobs": ("blobs", 70, 480, 854)}


def fill_phase(repeats, calls):
    import numpy as np
    import torch
    from frame_masks_throughput import _timed
    from index_components_throughput import _host_ms, content, host_filter
    from s2d_amd import ops
    from tests.index_fill_refs import frame_ring, ref_fill_holes
    res = {"min_area": MIN_AREA, "keep_largest": True, "fill_holes": "all", "tile": list(ops.component_tile())}
    for name, (kind, N, H, W) in CASES.items():
        index, conn = (frame_ring(H, W), 8) if kind == "ring" else content("blobs", N, H, W)
        dev = torch.from_numpy(index).to("cuda:0")
        mid, removed = ops.filter_components(dev, MIN_AREA, True, conn)
        out, filled = ops.fill_index_holes(mid, "all", conn)
        host_mid = host_filter(index, MIN_AREA, True, conn)
        assert np.array_equal(mid.cpu().numpy(), host_mid), name
        want, want_filled, _ = ref_fill_holes(host_mid, "all", conn)
        assert np.array_equal(out.cpu().numpy(), want) and np.array_equal(filled.cpu().numpy(), want_filled), name
        row = {"connectivity": conn, "removed_pixels": int(removed.sum()), "filled_pixels": int(filled.sum()), "equal_to_host": True}
        del out, want

        def both():
            m, _ = ops.filter_components(dev, MIN_AREA, True, conn)
            return ops.fill_index_holes(m, "all", conn, out=m)

        row["label_filter_ms"] = round(_timed(lambda: ops.filter_components(dev, MIN_AREA, True, conn), repeats, calls)[0], 4)
        row["label_filter_fill_ms"] = round(_timed(both, repeats, calls)[0], 4)
        row["fill_ms"] = round(_timed(lambda: ops.fill_index_holes(mid, "all", conn), repeats, calls)[0], 4)
        row["fill_over_filter"] = round(row["fill_ms"] / row["label_filter_ms"], 2)
        row["host_scipy_fill_ms"] = round(_host_ms(lambda: ref_fill_holes(host_mid, "all", conn), repeats), 1)
        row["host_scipy_fill_ms_per_frame"] = round(row["host_scipy_fill_ms"] / N, 2)
        row["host_over_device"] = round(row["host_scipy_fill_ms"] / row["fill_ms"], 1)
        res[name] = row
        print(f"fill phase {name}: {row}", file=sys.stderr, flush=True)
        del dev, mid
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
    with tempfile.TemporaryDirectory() as root:
        img_root = _write_tree(root, frames)
        for per_call in (1, 8):
            row = {}
            for name, fill in (("off", 0), ("on", "all")):
                lines = []
                for i in range(repeats + 1):                            # the first run is the warm-up
                    lines.append(write_masks(cfg, model, img_root, os.path.join(root, f"masks_{per_call}_{name}_{i}"), 0.0, 50, per_call,
                                             threads=16, min_component_area=MIN_AREA, keep_largest=True, fill_holes=fill))
                    print(f"driver run {i}, fill {name}, {per_call} frames per call: {lines[-1]}", file=sys.stderr, flush=True)
                timed = lines[1:]
                row[name] = {"frames": timed[0]["frames"], "removed_pixels": timed[0]["removed_pixels"],
                             "filled_pixels": timed[0]["filled_pixels"],
                             "frames_per_s": round(statistics.median(l["frames_per_s"] for l in timed), 1),
                             "runs_frames_per_s": [l["frames_per_s"] for l in timed]}
            res[f"frames_per_call_{per_call}"] = row
    return res


def measure(repeats, frames, calls):
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this script measures on an MI355X only")
    return {"device": torch.cuda.get_device_name(0), "repeats": repeats, "calls_per_timing": calls,
            "fill": fill_phase(repeats, calls), "driver": driver_phase(frames, repeats)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--frames", type=int, default=24, help="frames per sequence of the synthetic tree")
    ap.add_argument("--calls", type=int, default=20, help="back-to-back calls per kernel timing")
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
