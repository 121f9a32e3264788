"""Stage 1 of the recipe: one colour pseudo-mask PNG per video frame, the tree keymask discovery reads.

    python -m s2d_amd.keymask.frame_masks --config-file X.yaml --weights W.pth \\
        --video-base-path D/DAVIS/JPEGImages/480p --mask-base-path M \\
        [--confidence-threshold 0.35] [--max-masks 50] [--frames-per-call 1] [--job-id J --videos-per-job N] [--overwrite]
        [--threads 8] [--prefetch 2] [--dataset-name NAME]
        [--min-component-area N] [--keep-largest] [--component-connectivity {4,8}] [--fill-holes N|all] [KEY VALUE ...]

Restates what model_training/cutler/demo/demo.py does with its image model for this project's own checkpoint (one trained on image
annotations as pseudo-clips, `train --train-format coco_image`, or any other): the instances scored at least
--confidence-threshold are painted on black in descending order of their area in that frame, one fixed colour per instance index
(CustomVisualizer.draw_instance_predictions_on_black / overlay_masks_numpy, cutler/demo/predictor.py:237-355), and written as
M/<video>/<frame stem>.png, RGB, at the frame's original size; a frame with no instance is a black PNG.  The paint rule is
ops.paint_frames' (s2d_amd/frame_paint.py): straight from the mask logits, without mask planes.

The video folders are the sorted sub-directories of D, sliced per job by discover.video_and_mask_dirs; the frames of a folder are
discover.make_paths' images in its order for the dataset, so frame i of discovery pairs with mask i.  Each run of --frames-per-call
consecutive frames is one clip through `model([inputs])` with the model's inference_paint switch: 1 is the reference's per-image
behaviour; a larger value gives one set of proposals -- one colour per object -- per clip (the last clip of a video may be
shorter).  Decode, PIL-exact resize and prefetch are the test loader's; PNG encoding runs on a pool of at most 16 threads beside
the next clip's inference.  A video whose mask folder already holds a PNG for every frame is skipped unless --overwrite.

Where this differs from the reference, on purpose: the colours are the project's own table (ops.mask_colors: the DAVIS palette's
entries 1..n) and not detectron2's; equal areas are painted in proposal order (a stable sort) where numpy's argsort leaves the
order open; more instances than colours are cut to the first --max-masks instead of an IndexError past 50; --frames-per-call.

--min-component-area N (default 0), --keep-largest and --component-connectivity {4,8} (default 8) clean the painted owner map before
the PNGs are written (ops.filter_components, s2d_amd/index_components.py): of every instance's pixels in a frame, a connected
component smaller than N pixels is removed, and with --keep-largest every component but the instance's largest in that frame (equal
areas: the one whose first pixel comes first in raster order).  A removed pixel becomes black even where a larger instance painted
underneath also holds it: the plane-free paint keeps no second owner.  With the defaults no component kernel is launched and every
output byte is as before.

--fill-holes N|all (default 0: off) then fills the holes of the cleaned owner map (ops.fill_index_holes): a region of at most N black
pixels that does not touch the frame border and is enclosed by ONE instance -- the hole a removed speckle of another instance leaves
in the larger one it sat on -- takes that instance's id and colour.  The black pixels are connected under the connectivity
complementary to --component-connectivity; a region that borders two or more instances stays black.  With 0 no fill kernel is
launched.

The run ends with one JSON line on stdout: videos (folders of this job), skipped, frames (written), masks (proposals with a
non-zero area, summed over frames), empty_frames (frames in which none has one), removed_pixels (pixels the component cleanup
blackened; 0 with it off), filled_pixels (pixels --fill-holes painted; 0 with it off), wall_s, frames_per_s, loader_wait_fraction, encode_s (seconds inside PNG encoding, summed over the pool's
threads)."""
import argparse
import json
import os
import sys
import threading
import time
from concurrent.futures import ThreadPoolExecutor

from ..index_components import fill_holes_argument
from .discover import _DATASETS, make_paths, video_and_mask_dirs

MAX_THREADS = 16


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description="Stage-1 frame masks: colour pseudo-mask PNGs for keymask discovery")
    ap.add_argument("--config-file", required=True)
    ap.add_argument("--weights", default=None, help="checkpoint (default: MODEL.WEIGHTS of the config)")
    ap.add_argument("--video-base-path", required=True, help="D: one sub-directory of frames per video")
    ap.add_argument("--mask-base-path", required=True, help="M: receives M/<video>/<frame stem>.png")
    ap.add_argument("--confidence-threshold", type=float, default=0.35, help="instances scored below it are not painted")
    ap.add_argument("--max-masks", type=int, default=50, help="instances painted per clip at most (<= 254)")
    ap.add_argument("--frames-per-call", type=int, default=1, help="consecutive frames that share one set of proposals")
    ap.add_argument("--job-id", type=int, default=0)
    ap.add_argument("--videos-per-job", type=int, default=-1)
    ap.add_argument("--overwrite", action="store_true", help="rewrite videos whose masks are complete")
    ap.add_argument("--threads", type=int, default=8, help="decode threads and PNG threads (<= 16 each)")
    ap.add_argument("--prefetch", type=int, default=2)
    ap.add_argument("--dataset-name", default=None, help="frame-order rule of discover.make_paths instead of the one detected in "
                                                         "--video-base-path (no dataset in the path: numeric stems, as DAVIS)")
    ap.add_argument("--min-component-area", type=int, default=0, help="connected components of an instance smaller than this are "
                                                                      "blackened (0: off)")
    ap.add_argument("--keep-largest", action="store_true", help="keep only the largest connected component of every instance per frame")
    ap.add_argument("--component-connectivity", type=int, choices=(4, 8), default=8, help="pixel connectivity of the components")
    ap.add_argument("--fill-holes", type=fill_holes_argument, default=0, metavar="N|all",
                    help="fill holes of at most N pixels that one instance encloses, after the cleanup (0: off)")
    ap.add_argument("opts", nargs=argparse.REMAINDER, help="config overrides KEY VALUE ...")
    return ap.parse_args(argv)


def dataset_rule(video_base_path, dataset_name=None):
    """the dataset name make_paths sorts by: the given one, else the one discover detects in the path, else "DAVIS" (numeric stems)"""
    if dataset_name is not None:
        return dataset_name
    return next((name for key, name in _DATASETS if key in video_base_path), "DAVIS")


def video_frames(video_dir, dataset_name="DAVIS"):
    """the frame files of one folder in discover.make_paths' order (the folder stands in for the label folder, whose list is
    not used)"""
    return [os.path.basename(p) for p in make_paths(video_dir, video_dir, dataset_name)[0]]


def mask_name(frame_file):
    return os.path.splitext(os.path.basename(frame_file))[0] + ".png"


def masks_complete(mask_dir, frames):
    return bool(frames) and all(os.path.isfile(os.path.join(mask_dir, mask_name(f))) for f in frames)


def folder_document(video_base_path, mask_base_path, frames_per_call=1, job_id=0, videos_per_job=-1, dataset_name=None,
                    overwrite=False):
    """-> (document, clips, counts): the test loader's document with one record per CLIP -- frames_per_call consecutive frames of one
    video folder, the last clip of a folder as short as it has to be --, clips = {record id: (mask folder, [mask file names])}, and
    counts = {"videos": folders of this job, "skipped": those whose masks are complete (no record; none with overwrite)}"""
    from PIL import Image
    if int(frames_per_call) < 1:
        raise ValueError(f"--frames-per-call {frames_per_call}: at least 1")
    rule = dataset_rule(video_base_path, dataset_name)
    vids, _ = video_and_mask_dirs(video_base_path, mask_base_path, job_id, videos_per_job)
    videos, clips, skipped = [], {}, 0
    for vdir in vids:
        name = os.path.basename(vdir)
        frames = video_frames(vdir, rule)
        mdir = os.path.join(mask_base_path, name)
        if not frames:
            raise FileNotFoundError(f"{vdir}: no .jpg, .jpeg or .png frames")
        if not overwrite and masks_complete(mdir, frames):
            skipped += 1
            continue
        with Image.open(os.path.join(vdir, frames[0])) as im:
            width, height = im.size
        for c0 in range(0, len(frames), int(frames_per_call)):
            part = frames[c0:c0 + int(frames_per_call)]
            rid = len(videos) + 1
            videos.append({"id": rid, "name": name, "file_names": [os.path.join(name, f) for f in part], "height": height,
                           "width": width, "length": len(part)})
            clips[rid] = (mdir, [mask_name(f) for f in part])
    return {"videos": videos}, clips, {"videos": len(vids), "skipped": skipped}


def write_frame_png(path, rgb):
    """u8 [H,W,3] numpy -> an RGB-mode PNG (cv2.imwrite of the reference's picture, channels in RGB order as discovery reads them)"""
    from PIL import Image
    if rgb.ndim != 3 or rgb.shape[2] != 3 or str(rgb.dtype) != "uint8":
        raise ValueError(f"{path}: a frame mask is uint8 [H, W, 3], not {rgb.dtype} {rgb.shape}")
    Image.fromarray(rgb).save(path)                                  # [H,W,3] u8: mode RGB


class _Writer:
    """PNG encoding beside the next clip's inference: a clip's picture is copied to a pinned buffer on the caller's stream, and every
    frame of it is one task of the pool, which waits for the copy's event"""

    def __init__(self, threads):
        self.pool = ThreadPoolExecutor(max(1, min(int(threads), MAX_THREADS)))
        self.futs, self.encode_s, self._lock = [], 0.0, threading.Lock()

    def _put(self, host, t, ev, path):
        ev.synchronize()
        t0 = time.perf_counter()
        write_frame_png(path, host[t].numpy())
        dt = time.perf_counter() - t0
        with self._lock:
            self.encode_s += dt

    def submit(self, rgb, mask_dir, names):
        import torch
        os.makedirs(mask_dir, exist_ok=True)
        host = torch.empty(rgb.shape, dtype=torch.uint8, pin_memory=True)
        host.copy_(rgb, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(rgb.device))
        self.futs += [self.pool.submit(self._put, host, t, ev, os.path.join(mask_dir, n)) for t, n in enumerate(names)]
        while len(self.futs) > 8 * MAX_THREADS:          # bounded: the pinned buffers of finished clips are let go
            self.futs.pop(0).result()

    def close(self):
        try:
            for fu in self.futs:
                fu.result()
        finally:
            self.pool.shutdown(wait=True)


def write_masks(cfg, model, video_base_path, mask_base_path, confidence_threshold=0.35, max_masks=50, frames_per_call=1, job_id=0,
                videos_per_job=-1, overwrite=False, threads=8, prefetch=2, dataset_name=None, device=None, min_component_area=0,
                keep_largest=False, component_connectivity=8, fill_holes=0):
    """every clip of folder_document through `model([inputs])` (eval mode, inference_paint) and its pictures to
    mask_base_path/<video>/<frame stem>.png -> the report dict of the module docstring.  The model's training mode and inference
    switches are restored afterwards."""
    import torch
    from ..data.test_loader import YTVISTestLoader
    from ..modeling.postprocess import paint_options
    paint = {"max_masks": int(max_masks), "score_threshold": float(confidence_threshold), "min_component_area": min_component_area,
             "keep_largest": keep_largest, "component_connectivity": component_connectivity, "fill_holes": fill_holes}
    paint_options(paint)                                              # refused before anything is listed or run
    device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    doc, clips, counts = folder_document(video_base_path, mask_base_path, frames_per_call, job_id, videos_per_job, dataset_name,
                                         overwrite)
    loader = YTVISTestLoader.from_config(cfg, doc, video_base_path, device=device, threads=threads, prefetch=prefetch, shard=False)
    switches = ("inference_rle", "inference_device_masks", "inference_index", "inference_paint")
    was_training, was = model.training, {s: getattr(model, s, None) for s in switches}
    model.eval()
    model.inference_rle, model.inference_device_masks, model.inference_index, model.inference_paint = False, False, None, paint
    frames = masks = empty = 0
    removed, filled = [], []                                          # device counts: read once, after the last clip
    writer = _Writer(threads)
    try:
        torch.cuda.synchronize(device)
        t0 = time.perf_counter()
        try:
            with torch.no_grad():
                for inputs in loader:
                    out = model([inputs])
                    mdir, names = clips[inputs["video_id"]]
                    writer.submit(out["pred_masks"], mdir, names)
                    if "pred_removed" in out:
                        removed.append(out["pred_removed"])
                    if "pred_filled" in out:
                        filled.append(out["pred_filled"])
                    T = len(names)
                    per_frame = [sum(1 for a in out["pred_areas"] if a[t] > 0) for t in range(T)]
                    frames += T
                    masks += sum(per_frame)
                    empty += sum(1 for n in per_frame if n == 0)
        finally:
            writer.close()
        torch.cuda.synchronize(device)
        wall = time.perf_counter() - t0
    finally:
        model.train(was_training)
        for s, v in was.items():
            setattr(model, s, v)
    return {**counts, "frames": frames, "masks": masks, "empty_frames": empty,
            "removed_pixels": sum(int(r.sum()) for r in removed), "filled_pixels": sum(int(f.sum()) for f in filled), "wall_s": round(wall, 4),
            "frames_per_s": round(frames / wall, 3) if wall > 0 else None,
            "loader_wait_fraction": round(loader.wait_s / wall, 4) if wall > 0 else None, "encode_s": round(writer.encode_s, 4)}


def main(argv=None):
    a = parse_args(argv)
    import torch
    from ..config import load_config
    from ..evaluate import build_model
    from ..modeling.postprocess import paint_options
    paint_options({"max_masks": a.max_masks, "score_threshold": a.confidence_threshold, "min_component_area": a.min_component_area,
                   "keep_largest": a.keep_largest, "component_connectivity": a.component_connectivity, "fill_holes": a.fill_holes})
    cfg = load_config(a.config_file, a.opts)
    device = torch.device("cuda", torch.cuda.current_device())
    model = build_model(cfg, a.weights or cfg.MODEL.WEIGHTS, device)
    line = write_masks(cfg, model, a.video_base_path, a.mask_base_path, a.confidence_threshold, a.max_masks, a.frames_per_call,
                       a.job_id, a.videos_per_job, a.overwrite, a.threads, a.prefetch, a.dataset_name, device, a.min_component_area,
                       a.keep_largest, a.component_connectivity, a.fill_holes)
    print(json.dumps(line), flush=True)
    return line


if __name__ == "__main__":
    main(sys.argv[1:])
