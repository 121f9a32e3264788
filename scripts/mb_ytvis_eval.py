"""Microbenchmark of the YTVIS evaluator (s2d_amd/ytvis_eval.py) on a YTVIS-val-shaped synthetic workload: per video 36 frames
at 720x1280, D = 10 predictions of the device inference kernels (the masks inference_video makes before its host copy), G = 5
ground-truth tracks as compressed RLE (shifted copies of half the predictions).  Reports wall time per process() call,
evaluate() time, and, for scale, the same IoUs from decoded numpy planes (the pycocotools-free host path) on a few videos.

    python scripts/mb_ytvis_eval.py [--videos 100] [--numpy-videos 2] [--out profiles/ytvis_eval/mb.json]

Kernel times per video: run under `rocprofv3 --kernel-trace --stats -d <dir> -o <name> -- python scripts/mb_ytvis_eval.py`.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import oracle_np as O  # noqa: E402
from s2d_amd import ops  # noqa: E402
from s2d_amd.rle import encode_video_predictions  # noqa: E402
from s2d_amd.ytvis_eval import YTVISEvaluator  # noqa: E402

T, H, W, Q, C, D, G = 36, 720, 1280, 100, 40, 10, 5
HP, WP, HM, WM = 736, 1280, 92, 160
DEV = "cuda:0"


def predictions(seed):
    """device masks u8 [D,T,H,W] + scores / labels of one synthetic video, through the inference kernels"""
    g = torch.Generator(device="cpu").manual_seed(seed)
    low = (torch.randn((Q, T, HM // 8, WM // 8), generator=g) * 4 - 1.0).to(DEV)
    ml = F.interpolate(low, size=(HM, WM), mode="bilinear", align_corners=False)           # smooth blobs (set-up only)
    ldq = (Q + 3) // 4 * 4
    pm = torch.zeros((T * HM * WM, ldq), device=DEV)
    pm[:, :Q] = ml.reshape(Q, -1).T
    cls = torch.randn((Q, C + 1), generator=g).to(DEV)
    scores, query, label = ops.infer_select(cls, D)
    masks, _ = ops.infer_masks(pm, (T, HM, WM), (HP, WP), (H, W), (H, W), query)
    return masks, scores.tolist(), label.tolist()


def ground_truth(n_videos):
    videos, anns = [], []
    for v in range(n_videos):
        masks, _, _ = predictions(1000 + v)
        gt = torch.roll(masks[:G], shifts=(4, -6), dims=(2, 3)).contiguous()
        rles = encode_video_predictions(gt)
        videos.append({"id": v + 1, "height": H, "width": W, "length": T})
        for k in range(G):
            anns.append({"id": len(anns) + 1, "video_id": v + 1, "category_id": k % C, "iscrowd": 0, "segmentations": rles[k],
                         "areas": [int(a) for a in gt[k].reshape(T, -1).sum(1).tolist()]})
    return {"videos": videos, "categories": [{"id": c, "name": str(c)} for c in range(C)], "annotations": anns}


def numpy_ious(masks, gt_segs):
    """host path for scale: decode the ground truth with the oracle, sum_t |d & g| / |d | g| on numpy bool planes"""
    d = masks.cpu().numpy().astype(bool)
    g = np.stack([np.stack([O.rle_decode(s).astype(bool) for s in track]) for track in gt_segs])
    ious = np.zeros((D, G))
    for i in range(D):
        for j in range(G):
            inter = np.logical_and(d[i], g[j]).sum()
            union = np.logical_or(d[i], g[j]).sum()
            ious[i, j] = inter / union if union else 0.0
    return ious


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--videos", type=int, default=100)
    ap.add_argument("--numpy-videos", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    t0 = time.perf_counter()
    doc = ground_truth(a.videos)
    t_setup = time.perf_counter() - t0
    ev = YTVISEvaluator(json_file=doc, distributed=False)
    ev.reset()
    per_call = []
    for v in range(a.videos):
        masks, scores, labels = predictions(1000 + v)
        torch.cuda.synchronize()
        t = time.perf_counter()
        ev.process([{"video_id": v + 1, "length": T}], {"pred_scores": scores, "pred_labels": labels, "pred_masks": masks})
        torch.cuda.synchronize()
        per_call.append(time.perf_counter() - t)
    t = time.perf_counter()
    res = ev.evaluate()
    t_eval = time.perf_counter() - t
    np_times, max_diff = [], 0.0
    for v in range(min(a.numpy_videos, a.videos)):
        masks, _, _ = predictions(1000 + v)
        segs = [x["segmentations"] for x in doc["annotations"] if x["video_id"] == v + 1]
        t = time.perf_counter()
        ref = numpy_ious(masks, segs)
        np_times.append(time.perf_counter() - t)
        max_diff = max(max_diff, float(np.abs(ref - ev._records[v]["ious"]).max()))
    warm = per_call[1:] if len(per_call) > 1 else per_call
    out = {"videos": a.videos, "T": T, "H": H, "W": W, "D": D, "G": G,
           "process_ms_median": 1e3 * float(np.median(warm)), "process_ms_p90": 1e3 * float(np.percentile(warm, 90)),
           "process_ms_first": 1e3 * per_call[0], "evaluate_s": t_eval, "setup_s": t_setup,
           "numpy_ious_ms_per_video": 1e3 * float(np.mean(np_times)) if np_times else None, "numpy_max_abs_iou_diff": max_diff,
           "segm": res.get("segm")}
    print(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
