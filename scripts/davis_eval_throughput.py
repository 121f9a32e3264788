#!/usr/bin/env python3
"""Throughput of the DAVIS J&F evaluator (csrc/davis_eval.hip, s2d_amd/davis_eval.py) on a DAVIS-val-shaped synthetic set: 30
sequences x 70 frames of 480 x 854, 3 objects (drifting discs, a void block) and 20 proposals (the objects shifted, under other
labels, plus 17 small discs), unsupervised task, index maps already on the device (no PNG decoding), in one run:

  * sequence_metrics per sequence: wall ms to the returned J / F arrays, every sequence timed `repeats` times after a warm-up
    pass over the set; median, minimum and maximum over the sequences' medians, and the whole set (sum of the medians);
  * each kernel on the first sequence's planes, ms by device events over `iters` launches: index planes (23 x 70 planes out),
    boundary maps and disk dilations (R = 8) of the 20 x 70 proposal planes, the three per-frame count calls' shape
    (20 x 3 x 70), plane areas; the dilation's algorithmic GB/s (every plane read once and written once);
  * the numpy reference (tests/davis_refs.py) on the first 4 frames of the first sequence, for scale.

    python scripts/davis_eval_throughput.py [--iters 20] [--repeats 5] [--limit 600] [--out profiles/davis_eval/throughput.json]

The measurement runs in a child process under a time limit; prints one JSON line."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SEQS, T, H, W = 30, 70, 480, 854
OBJECTS, PROPOSALS = 3, 20


def _discs(dev, cy, cx, r, vy, vx):
    import torch
    t = torch.arange(T, device=dev, dtype=torch.float32)[:, None, None]
    yy = torch.arange(H, device=dev, dtype=torch.float32)[None, :, None]
    xx = torch.arange(W, device=dev, dtype=torch.float32)[None, None, :]
    return ((yy - (cy + vy * t)) ** 2 + (xx - (cx + vx * t)) ** 2) < r * r


def sequence(seed, dev):
    """-> (gt, res) CUDA u8 index videos [T, H, W]"""
    import torch
    g = torch.Generator().manual_seed(seed)
    u = lambda n: torch.rand(n, generator=g).tolist()
    gt = torch.zeros((T, H, W), device=dev, dtype=torch.uint8)
    res = torch.zeros((T, H, W), device=dev, dtype=torch.uint8)
    labels = (torch.randperm(PROPOSALS, generator=g) + 1).tolist()
    for j in range(OBJECTS, PROPOSALS):
        a, b, c = u(3)
        res[_discs(dev, a * H, b * W, 8 + 25 * c, 0.0, 1.0)] = labels[j]
    for k in range(OBJECTS):
        a, b, c, d, e = u(5)
        cy, cx, r, vy, vx = (0.25 + 0.5 * a) * H, (0.25 + 0.5 * b) * W, 50 + 60 * c, 2 * d - 1, 2 * e - 1
        gt[_discs(dev, cy, cx, r, vy, vx)] = k + 1
        res[_discs(dev, cy + 2, cx - 3, r + 1, vy, vx)] = labels[k]
    gt[:, 60:110, 400:540] = 255
    return gt, res


def _events(fn, iters):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for timed in (False, True):
        torch.cuda.synchronize()
        e0.record()
        for _ in range(iters if timed else 3):
            out = fn()
        e1.record()
        torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters, out


def measure(iters, repeats):
    import numpy as np
    import torch
    from s2d_amd import davis_eval as D
    from s2d_amd.ytvis_eval import plane_areas
    from tests import davis_refs as R
    dev = torch.device("cuda", 0)
    radius = D.davis_bound_pix(H, W)
    res = {"device": torch.cuda.get_device_name(0), "set": {"sequences": SEQS, "frames": T, "size": [H, W], "objects": OBJECTS,
                                                              "proposals": PROPOSALS, "radius": radius},
           "iters": iters, "repeats": repeats}
    seqs = [sequence(s, dev) for s in range(SEQS)]
    for gt, rs in seqs:                                                 # warm-up: every shape of the timed window
        out = D.sequence_metrics(gt, rs)
    per = []
    for gt, rs in seqs:
        ts = []
        for _ in range(repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = D.sequence_metrics(gt, rs)
            torch.cuda.synchronize()
            ts.append(1e3 * (time.perf_counter() - t0))
        per.append(statistics.median(ts))
    res["sequence_metrics_ms"] = {"median": round(statistics.median(per), 2), "min": round(min(per), 2), "max": round(max(per), 2),
                                  "whole_set": round(sum(per), 1)}
    res["last_sequence"] = {"J-Mean": round(float(out["J"].mean()), 4), "F-Mean": round(float(out["F"].mean()), 4)}

    gt, rs = seqs[0]
    k = {}
    k["index_planes_gt_and_results"], _ = _events(lambda: (D.index_planes(gt, OBJECTS), D.index_planes(rs, PROPOSALS)), iters)
    pplanes, _ = D.index_planes(rs, PROPOSALS)
    gplanes, _ = D.index_planes(gt, OBJECTS)
    wpf = pplanes.shape[2]
    flat = pplanes.view(PROPOSALS * T, wpf)
    k["seg2bmap_proposals"], bnd = _events(lambda: D.seg2bmap_planes(flat, H, W), iters)
    k["disk_dilate_proposals"], dil = _events(lambda: D.disk_dilate_planes(bnd, H, W, radius), iters)
    gb = D.disk_dilate_planes(D.seg2bmap_planes(gplanes.view(OBJECTS * T, wpf), H, W), H, W, radius).view(OBJECTS, T, wpf)
    k["frame_cross_counts_20x3x70"], _ = _events(lambda: D.frame_cross_counts(bnd.view(PROPOSALS, T, wpf), gb), iters)
    k["plane_areas_proposals"], _ = _events(lambda: plane_areas(flat), iters)
    res["kernel_ms"] = {n: round(v, 4) for n, v in k.items()}
    nbytes = 2 * bnd.numel() * 4
    res["disk_dilate"] = {"planes": PROPOSALS * T, "bytes_read_plus_written": nbytes,
                          "GBps": round(nbytes / (k["disk_dilate_proposals"] * 1e-3) / 1e9, 1),
                          "set_fraction": round(float(plane_areas(dil).sum()) / (PROPOSALS * T * H * W), 4)}
    short = 4
    g4, r4 = gt[:short].cpu().numpy(), rs[:short].cpu().numpy()
    t0 = time.perf_counter()
    ref = R.sequence_ref(g4, r4)
    ref_s = time.perf_counter() - t0
    got = D.sequence_metrics(g4, r4)
    res["numpy_reference"] = {"frames": short, "seconds": round(ref_s, 2), "ms_per_frame": round(1e3 * ref_s / short, 1),
                              "equal": bool(np.array_equal(ref["J"], got["J"]) and np.array_equal(ref["F"], got["F"]))}
    res["device_ms_per_frame"] = round(statistics.median(per) / T, 3)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--limit", type=int, default=600, help="seconds for the measuring child process")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        print(json.dumps(measure(a.iters, a.repeats)), flush=True)
        return 0
    t0 = time.perf_counter()
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--iters", str(a.iters), "--repeats", str(a.repeats)],
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
