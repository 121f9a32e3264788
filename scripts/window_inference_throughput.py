#!/usr/bin/env python3
"""Long-video inference on synthetic 720 x 1280 frames (MI355X; KD config, seeded random weights): the one-clip path against
windowed inference (MODEL.MASK_FORMER.TEST.WINDOW_SIZE 16, WINDOW_OVERLAP 2), and the fused cross-window count kernel against the
composition of the existing mask ops.

  * clip ladder: model([inputs]) with the switch off at T = 8, 16, 32, 64, ... -- peak device memory (torch allocator: every
    buffer of the library comes from it) and time.  Each T runs in a fresh child process under its own time limit.  The ladder
    stops BEFORE the first T whose predicted peak (the line through the two previous points) exceeds 80 % of the device memory, or
    whose largest activation tensor (T * Hp/4 * Wp/4 * 256 floats) would pass 2^30 elements, i.e. 32-bit byte offsets: the limit
    is approached by arithmetic, never by provoking an allocation failure.  A child that fails ends the whole run.
  * windowed: the same T values (and, with --extra-windowed, a few longer ones) with the switch on: peak memory, ms per frame, and
    the share of the device time between HIP events around association (counts, IoU, solver, permutation) + column scatter.
  * counts: s2d_window_pair_counts at O = 2, 184 x 320, Q = 100 against gather planes + pack_mask_bits + mask_pair_counts on the 2Q
    set: warmed, median of --iters device-event timings each, the two alternated; the fused kernel's share of its byte floor
    (2 * n * ldq * 4 bytes) at 8 TB/s.

    python scripts/window_inference_throughput.py --out DIR [--iters 200] [--extra-windowed 128,256]

Prints one JSON line and writes DIR/window_inference_throughput.json."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
KD_CFG = os.path.join(ROOT, "tests", "golden", "kd_config.json")
H, W = 720, 1280
WINDOW, OVERLAP = 16, 2
TEST_KEYS = "MODEL.MASK_FORMER.TEST."
HBM_BYTES_PER_S = 8e12


def padded_height():
    return (H + 31) // 32 * 32


def child_video(T, windowed):
    import torch
    from s2d_amd import ops
    from s2d_amd.config import load_config
    from s2d_amd.modeling import window_inference as wi
    from s2d_amd.modeling.meta_arch import META_ARCH_REGISTRY
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    opts = ["INPUT.MIN_SIZE_TEST", str(H)]
    if windowed:
        opts += [TEST_KEYS + "WINDOW_INFERENCE", "True", TEST_KEYS + "WINDOW_SIZE", str(WINDOW), TEST_KEYS + "WINDOW_OVERLAP", str(OVERLAP)]
    cfg = load_config(KD_CFG, opts)
    torch.manual_seed(0)
    model = META_ARCH_REGISTRY.get(cfg.MODEL.META_ARCHITECTURE).from_config(cfg).to(dev).eval()
    model.inference_device_masks = True
    g = torch.Generator(device=dev).manual_seed(1)
    frames = torch.randint(0, 256, (T, 3, H, W), device=dev, dtype=torch.uint8, generator=g)
    inputs = [{"image": list(frames), "height": H, "width": W}]

    spans = []

    def bracket(fn):
        def run(*a, **k):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            r = fn(*a, **k)
            e.record()
            spans.append((s, e))
            return r
        return run

    if windowed:
        wi.associate = bracket(wi.associate)
        wi._track_permutation = bracket(wi._track_permutation)
        ops.window_scatter_columns = bracket(ops.window_scatter_columns)
    # warm-up: the one-clip path at the timed shape; the windowed one on W + O frames (the same kernels and window shapes)
    warm = [{"image": list(frames[:min(T, WINDOW + OVERLAP)] if windowed else frames), "height": H, "width": W}]
    with torch.no_grad():
        model(warm)
        torch.cuda.synchronize()
        del spans[:]
        torch.cuda.empty_cache()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        s.record()
        out = model(inputs)
        e.record()
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
    dev_ms = s.elapsed_time(e)
    stitch_ms = sum(a.elapsed_time(b) for a, b in spans)
    q = model.num_queries
    ldq = (q + 3) // 4 * 4
    res = {"T": T, "windowed": bool(windowed), "windows": model.last_windows, "wall_s": round(wall, 4), "device_ms": round(dev_ms, 2),
           "ms_per_frame": round(dev_ms / T, 3), "peak_allocated_MB": round(torch.cuda.max_memory_allocated() / 1e6, 1),
           "peak_reserved_MB": round(torch.cuda.max_memory_reserved() / 1e6, 1), "resident_before_MB": round(base / 1e6, 1),
           "stitched_buffer_MB": round(T * (padded_height() // 4) * (W // 4) * ldq * 4 / 1e6, 1) if model.last_windows > 1 else 0.0,
           "device_total_MB": round(torch.cuda.get_device_properties(dev).total_memory / 1e6, 1),
           "predictions": len(out["pred_scores"])}
    if windowed:
        res["stitch_ms"] = round(stitch_ms, 3)
        res["stitch_share"] = round(stitch_ms / dev_ms, 5)
    return res


def child_counts(iters):
    import numpy as np
    import torch
    from s2d_amd import ops
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    Q, ldq, n = 100, 100, 2 * 184 * 320
    g = torch.Generator(device=dev).manual_seed(2)
    a = torch.randn((n, ldq), device=dev, generator=g)
    b = torch.randn((n, ldq), device=dev, generator=g)

    def fused():
        return ops.window_pair_counts(a, b, Q)

    def composed():
        planes = torch.cat([(a[:, :Q] > 0).t(), (b[:, :Q] > 0).t()]).to(torch.uint8).contiguous()
        return ops.mask_pair_counts(ops.pack_mask_bits(planes))

    inter, area_a, area_b = fused()
    full = composed()
    same = bool(torch.equal(full[:Q, Q:], inter) and torch.equal(torch.diagonal(full)[:Q], area_a) and torch.equal(torch.diagonal(full)[Q:], area_b))
    planes = torch.cat([(a[:, :Q] > 0).t(), (b[:, :Q] > 0).t()]).to(torch.uint8).contiguous()
    fns = {"fused": fused, "composition": composed, "composition_without_gather": lambda: ops.mask_pair_counts(ops.pack_mask_bits(planes))}
    for fn in fns.values():
        for _ in range(10):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(iters):                                                 # alternated: drift hits all alike
        for k, fn in fns.items():
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            fn()
            e.record()
            e.synchronize()
            times[k].append(s.elapsed_time(e))
    nbytes = 2 * n * ldq * 4
    med = {k: float(np.median(v)) for k, v in times.items()}
    res = {"n": n, "Q": Q, "ldq": ldq, "iters": iters, "equal_counts": same, "bytes_read": nbytes,
           "floor_ms_at_8TBps": round(nbytes / HBM_BYTES_PER_S * 1e3, 5)}
    for k in fns:
        res[k + "_ms_median"] = round(med[k], 5)
        res[k + "_ms_min"] = round(float(np.min(times[k])), 5)
        res[k + "_ms_p90"] = round(float(np.percentile(times[k], 90)), 5)
    res["fused_GBps"] = round(nbytes / (med["fused"] * 1e-3) / 1e9, 1)
    res["fused_fraction_of_8TBps"] = round(nbytes / HBM_BYTES_PER_S * 1e3 / med["fused"], 4)
    return res


def run_child(args, limit):
    """one measurement in a fresh process under its own time limit -> its JSON line (None: it failed, and nothing more is started)"""
    cmd = [sys.executable, os.path.abspath(__file__), "--child"] + args
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=limit, cwd=ROOT)
    except subprocess.TimeoutExpired:
        print(f"child {args} exceeded {limit} s", file=sys.stderr, flush=True)
        return None
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    if r.returncode != 0 or not lines:
        print(f"child {args} failed with status {r.returncode}:\n{r.stderr[-3000:]}", file=sys.stderr, flush=True)
        return None
    res = json.loads(lines[-1])
    print(json.dumps(res), flush=True)
    return res


def largest_activation_elements(T):
    return T * (padded_height() // 4) * (W // 4) * 256


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--limit", type=int, default=420, help="seconds per child process")
    ap.add_argument("--extra-windowed", default="", help="comma-separated longer T values for the windowed path only")
    ap.add_argument("--child", nargs="+", default=None)
    a = ap.parse_args()
    if a.child:
        kind = a.child[0]
        res = child_counts(int(a.child[1])) if kind == "counts" else child_video(int(a.child[1]), kind == "windowed")
        print(json.dumps(res), flush=True)
        return 0

    res = {"H": H, "W": W, "window_size": WINDOW, "window_overlap": OVERLAP, "clip": [], "windowed": [], "stopped": None}
    ok = True
    T = 8
    while ok:
        if largest_activation_elements(T) > 2 ** 30:
            res["stopped"] = f"T = {T}: the largest activation tensor would hold {largest_activation_elements(T)} > 2^30 floats"
            break
        if len(res["clip"]) >= 2:
            p0, p1 = res["clip"][-2], res["clip"][-1]
            pred = p1["peak_allocated_MB"] + (p1["peak_allocated_MB"] - p0["peak_allocated_MB"]) / (p1["T"] - p0["T"]) * (T - p1["T"])
            if pred > 0.8 * p1["device_total_MB"]:
                res["stopped"] = f"T = {T}: predicted peak {pred:.0f} MB > 80 % of {p1['device_total_MB']:.0f} MB"
                break
        r = run_child(["clip", str(T)], a.limit)
        if r is None:
            ok = False
            res["stopped"] = f"T = {T}: the one-clip child failed"
            break
        res["clip"].append(r)
        T *= 2
    if ok:
        extra = [int(v) for v in a.extra_windowed.split(",") if v]
        for T in [c["T"] for c in res["clip"]] + extra:
            r = run_child(["windowed", str(T)], a.limit)
            if r is None:
                ok = False
                break
            res["windowed"].append(r)
    if ok:
        res["counts"] = run_child(["counts", str(a.iters)], a.limit)
        ok = res["counts"] is not None
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "window_inference_throughput.json"), "w") as fh:
            fh.write(line + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
