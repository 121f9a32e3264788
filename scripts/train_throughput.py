#!/usr/bin/env python3
"""Throughput of the training loader and driver (python -m s2d_amd.train) on a seeded synthetic YTVIS-like split at 720p.

    python scripts/train_throughput.py --out DIR [--videos 12] [--frames 24] [--iters 20] [--threads 8]
    rocprofv3 --kernel-trace --stats -d P -o run -- python scripts/train_throughput.py --out DIR --kernels-only

Writes JPEG videos with RLE tracks (compressed and uncompressed), a train JSON and a seeded KD checkpoint under DIR.  Config: the
shipped KD config (SAMPLING_FRAME_NUM 3, IMS_PER_BATCH 4, crop + brightness / contrast / rotation).  Prints one JSON line:
  loader      ms per clip of the loader on its own (batches drawn back to back, nothing else on the GPU)
  training    iteration ms and loader wait fraction inside real training iterations (the driver's summary line; the first
              iterations include warm-up, so --iters should be well above 5)
  kernels     device ms (events) of one clip's masks through s2d_aug_warp_mask_bits vs bit unpack + s2d_aug_warp_masks_u8,
              and of its frames through s2d_aug_warp_frames_hwc_u8 vs permute + s2d_aug_warp_frames_u8
--kernels-only runs one loader batch and one pass of each kernel form (for a rocprofv3 kernel trace)."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
KD_CFG = os.path.join(ROOT, "tests", "golden", "kd_config.json")


def write_split(root, videos, frames, h, w, tracks=4, seed=0):
    import torch
    from PIL import Image
    from s2d_amd.rle import encode_video_predictions
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    vids, anns, aid = [], [], 0
    for v in range(1, videos + 1):
        os.makedirs(os.path.join(root, f"v{v:03d}"), exist_ok=True)
        names = []
        cs = rng.uniform(0.2, 0.8, (tracks, 2))
        masks = np.zeros((tracks, frames, h, w), np.uint8)
        for t in range(frames):
            img = np.stack([(xx // 4 + 3 * t) % 256, (yy // 3 + 17 * v) % 256, (xx + yy) % 256], -1).astype(np.int32)
            for k, (cx, cy) in enumerate(cs):
                blob = ((xx / w - cx - 0.004 * t) ** 2 + (yy / h - cy) ** 2) < 0.01 * (k + 1)
                masks[k, t] = blob
                img[blob, k % 3] = 40 * k + 60
            img = np.clip(img + rng.integers(-12, 12, img.shape), 0, 255).astype(np.uint8)
            name = f"v{v:03d}/{t:05d}.jpg"
            Image.fromarray(img).save(os.path.join(root, name), quality=90)
            names.append(name)
        vids.append({"id": v, "height": h, "width": w, "length": frames, "file_names": names})
        segs = encode_video_predictions(torch.from_numpy(masks).cuda())
        for k in range(tracks):
            s = segs[k]
            if k % 2:                                                   # every other track as uncompressed counts
                s = []
                for t in range(frames):
                    flat = masks[k, t].T.reshape(-1)
                    edges = np.flatnonzero(np.diff(np.concatenate([[0], flat, [1 - flat[-1]]])))
                    s.append({"size": [h, w], "counts": np.diff(np.concatenate([[0], edges])).tolist()})
            aid += 1
            anns.append({"id": aid, "video_id": v, "category_id": 1, "iscrowd": 0, "segmentations": s,
                         "bboxes": [[0, 0, 1, 1]] * frames, "areas": [int(masks[k, t].sum()) for t in range(frames)]})
    doc = {"info": {}, "licenses": [], "categories": [{"id": 1, "name": "object"}], "videos": vids, "annotations": anns}
    path = os.path.join(root, "train.json")
    with open(path, "w") as fh:
        json.dump(doc, fh)
    return path


def write_checkpoint(path, seed=0):
    import torch
    from s2d_amd.config import load_config
    from s2d_amd.modeling.meta_arch import META_ARCH_REGISTRY
    cfg = load_config(KD_CFG)
    torch.manual_seed(seed)
    model = META_ARCH_REGISTRY.get(cfg.MODEL.META_ARCHITECTURE).from_config(cfg)
    torch.save({"model": model.state_dict()}, path)


def _ev_ms(fn, reps=5):
    import torch
    fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def kernel_compare(cfg, records, reps=5):
    """one clip's masks and frames through the new kernels and through the two-step forms"""
    import random
    import torch
    from s2d_amd._lib import lib
    from s2d_amd.data.augment import augment_frames_hwc, warp_mask_bits
    from s2d_amd.data.train_loader import ClipSettings, _read_frames, _stage_frames, plan_clip
    from s2d_amd.ytvis_eval import decode_frames
    st = ClipSettings(cfg)
    plan = plan_clip(records[0], random.Random(0), np.random.RandomState(0), st)
    H0, W0 = records[0]["height"], records[0]["width"]
    H1, W1 = plan["out_hw"]
    T, S = plan["plane_of"].shape
    x = _stage_frames(plan, _read_frames(plan, None, st.fmt)).cuda()
    p = torch.from_numpy(plan["params"]).cuda()
    bits = decode_frames(plan["segs"], H0, W0)
    po = torch.from_numpy(plan["plane_of"]).cuda().long()
    sh = torch.arange(32, device="cuda", dtype=torch.int32)
    stream = torch.cuda.current_stream().cuda_stream

    def fused():
        warp_mask_bits(bits, plan["plane_of"], H0, W0, p, (H1, W1))

    def two_step():
        u8 = ((bits[:, :, None] >> sh) & 1).to(torch.uint8).view(bits.shape[0], -1)[:, :H0 * W0].view(-1, H0, W0)
        u8 = torch.cat([u8, torch.zeros((1, H0, W0), device="cuda", dtype=torch.uint8)])   # row -1: the dummy slot
        m = u8[po.T.reshape(-1)].view(S, T, H0, W0).contiguous()
        out = torch.empty((S, T, H1, W1), device="cuda", dtype=torch.uint8)
        lib().call("s2d_aug_warp_masks_u8", m, S, T, H0, W0, p, H1, W1, out, stream)

    def hwc():
        augment_frames_hwc(x, p, (H1, W1))

    def chw():
        out = torch.empty((T, 3, H1, W1), device="cuda", dtype=torch.uint8)
        lib().call("s2d_aug_warp_frames_u8", x.permute(0, 3, 1, 2).contiguous(), T, H0, W0, p, H1, W1, out, stream)

    return {"clip": {"T": T, "S": S, "in": [H0, W0], "out": [H1, W1]},
            "mask_bits_fused_ms": round(_ev_ms(fused, reps), 4), "unpack_plus_warp_masks_u8_ms": round(_ev_ms(two_step, reps), 4),
            "frames_hwc_ms": round(_ev_ms(hwc, reps), 4), "permute_plus_frames_chw_ms": round(_ev_ms(chw, reps), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--videos", type=int, default=12)
    ap.add_argument("--frames", type=int, default=24)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--loader-batches", type=int, default=12)
    ap.add_argument("--threads", type=int, default=8)
    ap.add_argument("--kernels-only", action="store_true")
    a = ap.parse_args()
    import torch
    from s2d_amd.config import load_config
    from s2d_amd.data.train_loader import YTVISTrainLoader, load_ytvis_train
    os.makedirs(a.out, exist_ok=True)
    path = os.path.join(a.out, "train.json")
    if not os.path.exists(path):
        path = write_split(a.out, a.videos, a.frames, a.height, a.width)
    cfg = load_config(KD_CFG)
    records = load_ytvis_train(path, a.out)
    if a.kernels_only:
        loader = YTVISTrainLoader.from_config(cfg, records, seed=0, device="cuda", threads=a.threads)
        it = iter(loader)
        next(it)
        it.close()
        torch.cuda.synchronize()
        print(json.dumps({"kernels": kernel_compare(cfg, records, reps=1)}), flush=True)
        return

    loader = YTVISTrainLoader.from_config(cfg, records, seed=0, device="cuda", threads=a.threads)
    it = iter(loader)
    next(it)                                                            # warm-up: library load, pinned pool
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    clips = 0
    for _ in range(a.loader_batches):
        clips += len(next(it))
    torch.cuda.synchronize()
    ms_per_clip = (time.perf_counter() - t0) * 1e3 / clips
    it.close()
    report = {"videos": a.videos, "frames_per_video": a.frames, "size": [a.height, a.width], "threads": a.threads,
              "clips_per_batch": int(cfg.SOLVER.IMS_PER_BATCH), "frames_per_clip": int(cfg.INPUT.SAMPLING_FRAME_NUM),
              "loader": {"batches": a.loader_batches, "ms_per_clip": round(ms_per_clip, 3)}}
    report["kernels"] = kernel_compare(cfg, records)

    ckpt = os.path.join(a.out, "ckpt.pth")
    if not os.path.exists(ckpt):
        write_checkpoint(ckpt)
    cmd = [sys.executable, "-m", "s2d_amd.train", "--config-file", KD_CFG, "--train-json", path, "--image-root", a.out,
           "--output-dir", os.path.join(a.out, "train"), "--weights", ckpt, "--threads", str(a.threads),
           "SOLVER.MAX_ITER", str(a.iters), "SOLVER.CHECKPOINT_PERIOD", "100000", "SEED", "0"]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT, timeout=1800)
    if r.returncode != 0:
        sys.stderr.write(r.stderr[-4000:])
        sys.exit(r.returncode)
    line = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{") and "iterations" in l][-1]
    report["training"] = {"iterations": line["iterations"], "iteration_ms": round(line["wall_s"] * 1e3 / line["iterations"], 2),
                          "clips_per_s": line["clips_per_s"], "loader_wait_fraction": line["loader_wait_fraction"]}
    print(json.dumps(report), flush=True)


if __name__ == "__main__":
    main()
