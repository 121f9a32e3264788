#!/usr/bin/env python3
"""Throughput of the DAVIS checkpoint driver (`python -m s2d_amd.evaluate --test-format davis`), in one run:

  * index-map phase at DAVIS 480p: output 480 x 854, T = 70 and T = 100 frames, K = 20 proposals, logits at the size
    INPUT.MIN_SIZE_TEST 360 gives (360 x 640 input, padded 384 x 640, maps 96 x 160, Q = 100 columns).  `ops.infer_index` under
    both rules against the composition available without it: `ops.infer_masks` (the [K,T,oh,ow] byte planes) followed by a torch
    first-hit over the planes.  Milliseconds by device events (median of `repeats` after a warm-up) and
    torch.cuda.max_memory_allocated above the resident inputs, for each; the first-hit maps are checked equal.
  * whole driver: evaluate.main on a synthetic tree of 30 sequences x `--frames` frames of 480 x 854 JPEGs with 3 ground-truth
    objects, a seeded model (tests/golden/kd_config.json, random weights): frames/s and the loader-wait fraction of its timing
    line, median of `repeats` runs after a warm-up run.

    python scripts/davis_driver_throughput.py [--repeats 3] [--frames 24] [--limit 900] [--out profiles/davis_driver/throughput.json]

The measurement runs in a child process under a time limit; prints one JSON line."""
import argparse
import contextlib
import io
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H, W, K, Q = 480, 854, 20, 100
PADDED, IMG, HM, WM = (384, 640), (360, 640), 96, 160
SEQS = 30


def _timed(fn, repeats):
    """-> (median ms by device events, peak bytes above what was allocated before, last result)"""
    import torch
    fn()
    torch.cuda.synchronize()
    ms, peak = [], 0
    for _ in range(repeats):
        out = None
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
        peak = max(peak, torch.cuda.max_memory_allocated() - base)
    return statistics.median(ms), peak, out


def index_phase(T, repeats):
    import torch
    from s2d_amd import ops
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(T)
    coarse = torch.randn((Q * T, 1, 6, 6), device=dev, generator=g) * 3.0
    planes = torch.nn.functional.interpolate(coarse, size=(HM, WM), mode="bicubic", align_corners=True)[:, 0]
    ml = planes.view(Q, T * HM * WM).t().contiguous()
    query = torch.randperm(Q, device=dev, generator=g)[:K].to(torch.int32).contiguous()
    score = torch.sort(torch.rand(K, device=dev, generator=g), descending=True).values.contiguous()
    del coarse, planes
    dims, out = (T, HM, WM), (H, W)

    def composed():
        masks, _ = ops.infer_masks(ml, dims, PADDED, IMG, out, query)
        hold = masks != 0
        return torch.where(hold.any(0), hold.int().argmax(0) + 1, 0).to(torch.uint8)

    res = {}
    for rule in ("rank", "prob"):
        ms, peak, idx = _timed(lambda: ops.infer_index(ml, dims, PADDED, IMG, out, query, score, rule), repeats)
        res[f"infer_index_{rule}"] = {"ms": round(ms, 3), "peak_bytes": int(peak)}
        if rule == "rank":
            rank = idx
    ms, peak, ref = _timed(composed, repeats)
    res["infer_masks_plus_torch_first_hit"] = {"ms": round(ms, 3), "peak_bytes": int(peak)}
    ms, peak, _ = _timed(lambda: ops.infer_masks(ml, dims, PADDED, IMG, out, query), repeats)
    res["infer_masks_alone"] = {"ms": round(ms, 3), "peak_bytes": int(peak)}
    res["rank_equals_composition"] = bool(torch.equal(rank, ref))
    res["index_bytes"] = T * H * W
    res["unlabelled_share"] = round(float((rank == 0).float().mean()), 4)
    return res


def _write_tree(root, frames):
    import numpy as np
    from PIL import Image
    from s2d_amd.davis_eval import save_index_png
    rng = np.random.default_rng(0)
    img_root, gt_dir = os.path.join(root, "JPEGImages", "480p"), os.path.join(root, "Annotations_unsupervised", "480p")
    yy, xx = np.mgrid[0:H, 0:W]
    base = rng.integers(0, 255, (H, W, 3), dtype=np.uint8)
    for s in range(SEQS):
        name = f"seq{s:02d}"
        os.makedirs(os.path.join(img_root, name))
        os.makedirs(os.path.join(gt_dir, name))
        for t in range(frames):
            Image.fromarray(np.roll(base, (s * 7 + t * 3) % W, axis=1)).save(os.path.join(img_root, name, f"{t:05d}.jpg"), quality=85)
            gt = np.zeros((H, W), np.uint8)
            for k in range(3):
                cy, cx = 120 + 110 * k + t, 200 + 200 * k - 2 * t
                gt[(yy - cy) ** 2 + (xx - cx) ** 2 < (50 + 10 * k) ** 2] = k + 1
            save_index_png(os.path.join(gt_dir, name, f"{t:05d}.png"), gt)
    return img_root, gt_dir


def driver_phase(frames, repeats):
    import torch
    from s2d_amd import evaluate
    from s2d_amd.checkpoint import kd_to_plain
    from s2d_amd.config import load_config
    from s2d_amd.modeling.meta_arch import META_ARCH_REGISTRY
    cfg_path = os.path.join(ROOT, "tests", "golden", "kd_config.json")
    with tempfile.TemporaryDirectory() as root:
        t0 = time.perf_counter()
        img_root, gt_dir = _write_tree(root, frames)
        tree_s = time.perf_counter() - t0
        cfg = load_config(cfg_path, [])
        torch.manual_seed(0)
        model = META_ARCH_REGISTRY.get(cfg.MODEL.META_ARCHITECTURE).from_config(cfg)
        ckpt = os.path.join(root, "model.pth")
        torch.save({"model": kd_to_plain({k: v.detach().cpu() for k, v in model.state_dict().items()}), "iteration": 0}, ckpt)
        del model
        lines = []
        for i in range(repeats + 1):                                    # the first run is the warm-up
            buf = io.StringIO()
            with contextlib.redirect_stdout(buf):
                evaluate.main(["--config-file", cfg_path, "--gt", gt_dir, "--image-root", img_root, "--output-dir", os.path.join(root, f"out{i}"),
                               "--weights", ckpt, "--threads", "16", "--test-format", "davis", "MODEL.MASK_FORMER.TEST.NUM_PREDICTIONS", "20"])
            lines.append(json.loads([l for l in buf.getvalue().splitlines() if l.startswith("{")][-1]))
        with open(os.path.join(root, f"out{repeats}", "metrics.json")) as fh:
            metrics = json.load(fh)
    timed = lines[1:]
    return {"sequences": SEQS, "frames_per_sequence": frames, "frames": timed[0]["frames"], "size": [H, W], "tree_write_s": round(tree_s, 1),
            "frames_per_s": round(statistics.median(l["frames_per_s"] for l in timed), 1),
            "wall_s": round(statistics.median(l["wall_s"] for l in timed), 2),
            "loader_wait_fraction": round(statistics.median(l["loader_wait_fraction"] for l in timed), 4),
            "runs": [{k: l[k] for k in ("frames_per_s", "wall_s", "loader_wait_fraction")} for l in timed],
            "J&F-Mean_random_weights": round(metrics["davis"]["J&F-Mean"], 4)}


def measure(repeats, frames):
    import torch
    res = {"device": torch.cuda.get_device_name(0), "repeats": repeats,
           "index_map_phase": {"output": [H, W], "K": K, "maps": [HM, WM], "padded": list(PADDED), "image": list(IMG), "ldq": Q}}
    for T in (70, 100):
        res["index_map_phase"][f"T{T}"] = index_phase(T, repeats)
    res["driver"] = driver_phase(frames, repeats)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--frames", type=int, default=24, help="frames per sequence of the synthetic tree")
    ap.add_argument("--limit", type=int, default=900, help="seconds for the measuring child process")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.repeats < 3:
        ap.error("medians of at least 3")
    if a.child:
        print(json.dumps(measure(a.repeats, a.frames)), flush=True)
        return 0
    t0 = time.perf_counter()
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--repeats", str(a.repeats), "--frames", str(a.frames)],
                           capture_output=True, text=True, timeout=a.limit, cwd=ROOT)
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
