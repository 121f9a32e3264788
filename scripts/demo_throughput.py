#!/usr/bin/env python3
"""Video demo stage times on a synthetic 36-frame 720p video (MI355X), for K = 10 and K = 50 kept instances:

  * decode_s: demo.decode_frames of the 36 JPEG frames (pool of 16 threads);
  * model_s: model([inputs]) of the KD config (random weights, device masks), warmed;
  * areas / render kernels: device time by torch.cuda.Event around warmed launches, and GB/s against the byte floor of the u8
    layout (areas: K*T*H*W mask bytes; render: frames in + masks in + overlay out + index map out);
  * d2h_s: the overlay and index map copied to pinned host memory (one copy each, events);
  * write_s: demo.write_outputs (JPEG overlays + palette mask PNGs, 16 writer threads, chunked copies);
  * host_numpy_render_s_per_frame: demo.render_host on 3 frames, per frame (the comparison the device pass replaces).

    python scripts/demo_throughput.py [--iters 20] [--out DIR]

Prints one JSON line (and writes DIR/demo_throughput.json)."""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from s2d_amd import demo, ops  # noqa: E402

T, H, W = 36, 720, 1280
KD_CFG = os.path.join(ROOT, "tests", "golden", "kd_config.json")


def synthetic_frames(rng):
    yy, xx = np.mgrid[0:H, 0:W]
    base = np.stack([(xx // 5) % 256, (yy // 3) % 256, ((xx + yy) // 7) % 256], -1).astype(np.int32)
    return np.stack([np.clip(base + rng.integers(-30, 30, base.shape) + 3 * t, 0, 255).astype(np.uint8) for t in range(T)])


def synthetic_masks(K, dev):
    m = torch.zeros((K, T, H, W), dtype=torch.uint8, device=dev)
    for k in range(K):
        for t in range(T):
            y, x = (37 * k + 11 * t) % (H - 260), (97 * k + 23 * t) % (W - 400)
            m[k, t, y:y + 120 + 2 * k, x:x + 180 + 3 * k] = 1
    return m


def timed(fn, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn()
    torch.cuda.synchronize()
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / iters / 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    rng = np.random.default_rng(0)
    frames_h = synthetic_frames(rng)
    work = tempfile.mkdtemp(prefix="demo_tp")
    res = {"T": T, "H": H, "W": W}
    try:
        from PIL import Image
        vdir = os.path.join(work, "frames", "clip")
        os.makedirs(vdir)
        files = []
        for t in range(T):
            files.append(os.path.join(vdir, f"{t:05d}.jpg"))
            Image.fromarray(frames_h[t]).save(files[-1], quality=90)
        t0 = time.perf_counter()
        host = demo.decode_frames(files)
        res["decode_s"] = round(time.perf_counter() - t0, 4)
        frames = host.to(dev)

        from s2d_amd.config import load_config
        from s2d_amd.modeling.meta_arch import META_ARCH_REGISTRY
        cfg = load_config(KD_CFG)
        torch.manual_seed(0)
        model = META_ARCH_REGISTRY.get(cfg.MODEL.META_ARCHITECTURE).from_config(cfg).to(dev).eval()
        model.inference_device_masks = True
        with torch.no_grad():
            model([demo.model_inputs(cfg, frames)])
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            model([demo.model_inputs(cfg, frames)])
            torch.cuda.synchronize()
        res["model_s"] = round(time.perf_counter() - t0, 4)
        del model
        torch.cuda.empty_cache()

        per_k = {}
        for K in (10, 50):
            masks = synthetic_masks(K, dev)
            colors = torch.from_numpy(demo.instance_colors(K)).to(dev)
            _, order = ops.mask_frame_areas(masks)
            areas_s = timed(lambda: ops.mask_frame_areas(masks), a.iters)
            render_s = timed(lambda: ops.render_instances(frames, masks, order, colors, demo.ALPHA, want_index=True), a.iters)
            px = T * H * W
            areas_bytes = K * px
            render_bytes = 3 * px + K * px + 3 * px + px
            overlay, index = ops.render_instances(frames, masks, order, colors, demo.ALPHA, want_index=True)
            ov_h = torch.empty(overlay.shape, dtype=torch.uint8, pin_memory=True)
            ix_h = torch.empty(index.shape, dtype=torch.uint8, pin_memory=True)
            d2h_s = timed(lambda: (ov_h.copy_(overlay, non_blocking=True), ix_h.copy_(index, non_blocking=True)), 3)
            out = os.path.join(work, f"out{K}")
            os.makedirs(out)
            t0 = time.perf_counter()
            demo.write_outputs(overlay, index, files, out)
            write_s = time.perf_counter() - t0
            fr3 = frames_h[:3]
            m3 = masks[:, :3].cpu().numpy()
            t0 = time.perf_counter()
            demo.render_host(fr3, m3, demo.instance_colors(K))
            host_s = (time.perf_counter() - t0) / 3
            per_k[str(K)] = {"areas_ms": round(areas_s * 1e3, 4), "areas_GBps": round(areas_bytes / areas_s / 1e9, 1),
                             "render_ms": round(render_s * 1e3, 4), "render_floor_MB": round(render_bytes / 1e6, 1),
                             "render_GBps": round(render_bytes / render_s / 1e9, 1),
                             "render_floor_ms_at_6300GBps": round(render_bytes / 6.3e12 * 1e3, 4),
                             "d2h_s": round(d2h_s, 4), "write_s": round(write_s, 4),
                             "host_numpy_render_s_per_frame": round(host_s, 4)}
            del masks, overlay, index
            torch.cuda.empty_cache()
        res["K"] = per_k
    finally:
        shutil.rmtree(work, ignore_errors=True)
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "demo_throughput.json"), "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
