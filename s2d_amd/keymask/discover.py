"""Keymask discovery: colour pseudo-mask PNGs + a point tracker -> one YTVIS-style annotation JSON per video.

    python -m s2d_amd.keymask.discover --video-base-path D/DAVIS/JPEGImages/480p --mask-base-path M --save-path S \\
        --visibility-maps-output-base V --visibility-clusters-output-base C --annotation-output-path A \\
        --tracker cotracker --tracker-checkpoint scaled_offline.pth          (or --tracker block: the built-in baseline;
                                  or --tracker block-live [--tracker-options search=48,refresh=-1]: wide search, live template;
                                  or --tracker block-zm [--tracker-options search=48,texture=0]: zero-mean cost, texture gate)

The mask tree M/<video>/<frame>.png is stage 1's output: `python -m s2d_amd.keymask.frame_masks` writes it from a checkpoint of this
project (any other tree of one colour PNG per frame, such as the reference's cutler/demo output, reads the same).

Restates keymask_ident/main_keymask_ident.py and its per-video stages with their file names, layouts, JSON contents and
observable quirks:

  1. visibility     cotracker_occlusions.py:243-396 extract_object_visibility_data: one tracker call per (frame, object),
                    grid 50, backward tracking from frame 1 on; <maps>/<dataset>/<split>/data/<video>.json
  2. windows        identify_visibility_windows.py:108-231: DBSCAN over the binarised curves (grouping.visibility_windows);
                    <clusters>/<dataset>/<split>/<video>.json
  3. cluster masks  crw_utils.py:796-857 load_frames_and_masks + keymask_utils.save_segmentation_masks:
                    <save>/<video>/cluster_<c>/cluster<c>_frame<f>_mask<m>.png
  4. matching       cotracker_matching.py:926-1136 temporal_correspondence_match: one tracker call per cluster mask in its
                    merged visibility range, grid max(min(area // 800, 50), 25); group_<g>/ trees, video_coverage.txt,
                    cluster_coverage.txt, one2x_data_cluster<c>.json, video_one2x_data.json
  5. annotation     annotations.py:8-139; <annotations>/<video>.json

Device side: each video's colour masks are decoded once (color_masks_to_ids) into one IdMap that all stages use; the query
masks come from s2d_idmap_select_masks_u8, the visibility curves from s2d_visibility_curve_f32 (read back once per video), and
each tracked mask's matches from s2d_track_point_id_counts (one read-back per tracked mask).  The cluster PNG tree is written
as in the reference, but the matching stage takes the masks it wrote from memory instead of reading them back.  DBSCAN runs
on the host (grouping.py).

Where this differs from the reference, on purpose:
  * the tracker is built once per run (the reference builds one per video and stage) and comes from --tracker;
  * temporal_correspondence_match falls off its end (returns None) after a full run, which makes the reference's
    `status > 0` raise; a completed matching stage counts as success here, -1 as "no valid annotations";
  * an exception in write_annotation_for_video counts as a failed video instead of ending the run;
  * frames are decoded once (PIL, RGB) and serve both tracker stages and the frame size of stage 3;
  * progress goes to stderr; the run ends with one JSON line on stdout.
"""
import argparse
import glob
import json
import os
import random
import sys
import time
import warnings

import numpy as np
import torch
from PIL import Image

from . import formats, grouping
from .propagate import IdMap, color_masks_to_ids, extract_mask_matches_from_tracks, visibility_curve
from .tracker import load_tracker

_DATASETS = (("DAVIS", "DAVIS"), ("ytvis2021", "ytvis2021"), ("ytvis2019", "ytvis2019"), ("ovis", "ovis"),
             ("VIPSeg", "VIPSeg"), ("MOSE", "MOSE"), ("sa-v", "SA-V"))


def parse_tracker_options(text):
    """'search=48,refresh=-1' -> {"search": 48, "refresh": -1}: comma-separated key=int"""
    out = {}
    for item in filter(None, (s.strip() for s in (text or "").split(","))):
        key, sep, value = (s.strip() for s in item.partition("="))
        try:
            if not sep or not key.isidentifier():
                raise ValueError
            out[key] = int(value)
        except ValueError:
            raise ValueError(f"--tracker-options {text!r}: expected key=int[,key=int...], got {item!r}") from None
    return out


def parse_args(argv=None):
    """crw_utils.keymask_args (same flags and defaults) + --tracker, --tracker-options, --tracker-checkpoint, --dataset-name"""
    p = argparse.ArgumentParser(description="Keymask Identification")
    p.add_argument("--workers", default=4, type=int, metavar="N", help="accepted for compatibility; unused")
    p.add_argument("--manualSeed", type=int, default=777, help="manual seed")
    p.add_argument("--gpu-id", default="0", type=str, help="accepted for compatibility; select the device with HIP_VISIBLE_DEVICES")
    p.add_argument("--batchSize", default=1, type=int, help="accepted for compatibility; unused")
    p.add_argument("--video-base-path", default="/mnt/data/datasets/DAVIS/JPEGImages/480p", type=str, help="Base path for videos")
    p.add_argument("--mask-base-path", default="/mnt/data/outputs/DAVIS/cuts3d/pseudo_annotations", type=str, help="Base path for masks")
    p.add_argument("--save-path", default="/mnt/data/outputs/cotracker/segmentation_masks/DAVIS/all/", type=str)
    p.add_argument("--video-output-dir", default="/mnt/data/outputs/cotracker/videos", type=str,
                   help="accepted for compatibility; videos are not written")
    p.add_argument("--visibility-maps-output-base", default="/mnt/data/outputs/cotracker/visibility_maps", type=str)
    p.add_argument("--visibility-clusters-output-base", default="/mnt/data/outputs/cotracker/visibility_clusters", type=str)
    p.add_argument("--annotation-output-path", default="/mnt/data/outputs/cotracker/annotations/DAVIS/all/", type=str)
    p.add_argument("--visibility-threshold", default=0.3, type=float, help="Threshold for visibility grouping")
    p.add_argument("--matching-threshold", default=0.5, type=float, help="Threshold for proxy propagate-and-match")
    p.add_argument("--job-id", default=0, type=int, help="Job ID for distributed training")
    p.add_argument("--videos-per-job", default=-1, type=int, help="Number of videos to process per job")
    p.add_argument("--debug", default=False, action="store_true", help="Debug mode")
    p.add_argument("--tracker", default="cotracker",
                   help="'cotracker', 'block' (the built-in block-matching baseline: no package, no weights), 'block-live' (the same "
                        "with a search of up to 64 px and a live template), 'block-zm' (that search with a zero-mean cost, which a "
                        "change of brightness does not disturb, and a texture gate) or 'pkg.module:factory'")
    p.add_argument("--tracker-options", default=None, metavar="KEY=INT[,KEY=INT...]",
                   help="keyword arguments of the built-in trackers, e.g. 'search=48,refresh=-1' (block: radius, search, tau; "
                        "block-live: radius, search, tau, refresh; block-zm: radius, search, tau, refresh, texture)")
    p.add_argument("--tracker-checkpoint", default=None, help="passed to the tracker (CoTracker: scaled_offline.pth)")
    p.add_argument("--dataset-name", default=None, help="dataset name instead of the one detected in --video-base-path")
    return p.parse_args(argv)


def _stage_split(path):
    """the split rule of the stage functions (cotracker_occlusions.py:281-292, cotracker_matching.py:961-972)"""
    for key in ("train", "valid", "test", "val", "imgs"):
        if key in path:
            return key
    return "all"


def _main_split(dataset_name, path):
    if dataset_name == "DAVIS":
        return "all"
    if dataset_name in ("ytvis2021", "ytvis2019", "ovis", "MOSE"):
        return "train" if "train" in path else "valid"
    if dataset_name == "VIPSeg":
        return "imgs"
    if dataset_name == "SA-V":
        return "train"
    return _stage_split(path)


def detect_dataset(video_base_path, dataset_name=None):
    """(dataset_name, split) of main_keymask_ident.py:40-76 from path substrings; dataset_name overrides the name (the split
    then follows that dataset's rule, or the stage rule for a name the reference does not know)"""
    if dataset_name is None:
        dataset_name = next((name for key, name in _DATASETS if key in video_base_path), None)
        if dataset_name is None:
            raise ValueError("Unknown dataset name. Please specify the dataset name in the video base path.")
    return dataset_name, _main_split(dataset_name, video_base_path)


def stage_dataset(video_path, dataset_name=None):
    """(dataset_name, split) as the per-video stages detect them (cotracker_occlusions.py:266-292)"""
    if dataset_name is None:
        dataset_name = next((name for key, name in _DATASETS if key in video_path), None)
        if dataset_name is None:
            raise ValueError("Unknown dataset")
    return dataset_name, _stage_split(video_path)


def video_and_mask_dirs(video_base_path, mask_base_path, job_id=0, videos_per_job=-1):
    """main_keymask_ident.py:14-36: both lists built from the sorted names under the video base, each filtered by its own
    isdir and sliced per job (so a missing mask folder shifts the pairing, as in the reference)"""
    names = sorted(os.listdir(video_base_path))
    vids = [p for p in (os.path.join(video_base_path, n) for n in names) if os.path.isdir(p)]
    masks = [p for p in (os.path.join(mask_base_path, n) for n in names) if os.path.isdir(p)]
    if videos_per_job > 0:
        start = job_id * videos_per_job if job_id > 0 else 0
        vids, masks = vids[start:start + videos_per_job], masks[start:start + videos_per_job]
    return vids, masks


def make_paths(folder_path, label_path, dataset_name="DAVIS"):
    """crw_utils.py:769-794, with its sort rules: numeric stem; SA-V and ovis sort the frames by the number after the first '_';
    for ovis the labels keep os.listdir order (the reference sorts the frames twice)"""
    I = [i for i in os.listdir(folder_path) if i.endswith((".jpg", ".png", ".jpeg"))]
    L = [x for x in os.listdir(label_path) if "npy" not in x]
    n = len(I)
    if dataset_name == "SA-V":
        I.sort(key=lambda x: int(x.split("_")[1].split(".")[0]))
        L.sort(key=lambda x: int(x.split("_")[1].split(".")[0]))
    elif dataset_name == "ovis":
        I.sort(key=lambda x: int(x.split("_")[1].split(".")[0]))
    else:
        I.sort(key=lambda x: int(x.split(".")[0]))
        L.sort(key=lambda x: int(x.split(".")[0]))
    return ["%s/%s" % (folder_path, I[i]) for i in range(n)], ["%s/%s" % (label_path, L[i]) for i in range(n)]


def _read_rgb(path):
    """cv2.imread(IMREAD_COLOR) + BGR2RGB: a 3-channel uint8 array, or None where the file cannot be decoded"""
    try:
        with Image.open(path) as im:
            return np.asarray(im.convert("RGB"))
    except (OSError, ValueError):
        return None


def load_video(img_folder):
    """mp4_from_images (cotracker_occlusions.py:87-128): *.png, *.jpg, *.jpeg, *.bmp sorted by path -> float [1,T,3,H,W] on the
    device"""
    paths = []
    for e in ("*.png", "*.jpg", "*.jpeg", "*.bmp"):
        paths.extend(glob.glob(os.path.join(img_folder, e)))
    if not paths:
        raise ValueError(f"No images found in {img_folder!r}")
    frames = [f for f in (_read_rgb(p) for p in sorted(paths)) if f is not None]
    if not frames:
        raise ValueError("None of the images could be read successfully.")
    return torch.from_numpy(np.stack(frames)).cuda().permute(0, 3, 1, 2)[None].float()


def load_idmap(mask_folder):
    """load_masks (cotracker_occlusions.py:22-84 == cotracker_matching.py:22-84) decoded once on the device; None where the
    folder holds no PNG (the reference warns and returns None)"""
    paths = sorted(glob.glob(os.path.join(mask_folder, "*.png")))
    if not paths:
        warnings.warn(f"No .png masks found in {mask_folder!r}")
        return None
    frames = [f for f in (_read_rgb(p) for p in paths) if f is not None]
    if not frames:
        raise RuntimeError("No valid mask images could be read.")
    return IdMap(color_masks_to_ids(torch.from_numpy(np.stack(frames)).cuda()))


def _mask_hw(mask):
    return torch.from_numpy(np.ascontiguousarray(mask))[None, None]


class _Run:
    """per-run state: the tracker (timed), arguments and counters"""

    def __init__(self, args, tracker):
        self.args, self.tracker = args, tracker
        self.tracker_s = 0.0

    def track(self, video, grid_size, grid_query_frame, segm_mask, backward_tracking):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = self.tracker(video, grid_size=grid_size, grid_query_frame=grid_query_frame, segm_mask=segm_mask,
                           backward_tracking=backward_tracking)
        torch.cuda.synchronize()
        self.tracker_s += time.perf_counter() - t0
        return out

    def log(self, *a):
        print(*a, file=sys.stderr)


def visibility_stage(run, video_path, idmap):
    """extract_object_visibility_data (cotracker_occlusions.py:243-396) -> ({"video_data": [...]} or None, the video)"""
    dataset_name, split = stage_dataset(video_path, run.args.dataset_name)
    out_dir = os.path.join(run.args.visibility_maps_output_base, dataset_name, split)
    os.makedirs(out_dir, exist_ok=True)
    video_name = os.path.basename(video_path)
    video = load_video(video_path)
    rows, curves = [], []
    for q in range(video.shape[1]):
        if q >= idmap.T:
            raise IndexError(f"index {q} is out of bounds for dimension 0 with size {idmap.T}")
        oids = [int(o) for o in idmap.frame_object_ids(q)]
        if not oids:
            continue
        masks = formats.select_masks(idmap.ids, [q] * len(oids), oids)
        data = []
        for oid, m in zip(oids, masks):
            _, vis = run.track(video, 50, q, _mask_hw(m), q > 0)
            # torch.mean over no points is NaN; the curve kernel writes nothing for P = 0
            curves.append(visibility_curve(vis) if vis.shape[-1] > 0 else torch.full((vis.shape[1],), float("nan"), device="cuda"))
            data.append(oid)
        rows.append((q, data))
    if not rows:
        return None, video
    host = torch.stack(curves).cpu().tolist()                           # one read-back per video
    it = iter(host)
    video_data = [{"frame_id": q, "data": [{"object_id": oid, "visibility": next(it)} for oid in data]} for q, data in rows]
    path = os.path.join(out_dir, "data", video_name + ".json")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        json.dump({"video_data": video_data}, f, indent=4)
    return {"video_data": video_data}, video


def windows_stage(visibility_data, dataset_name, split, video_name, cluster_output_dir, visibility_threshold):
    """get_visibility_windows_for_video (identify_visibility_windows.py:108-231)"""
    curves, row_ids = [], []
    for per_frame in visibility_data["video_data"]:
        for obj in per_frame["data"]:
            curves.append(obj["visibility"])
            row_ids.append({"frame_id": per_frame["frame_id"], "object_id": obj["object_id"]})
    video_data = {"video_name": video_name,
                  "clusters": grouping.visibility_windows(np.asarray(curves, np.float32), row_ids, visibility_threshold)}
    path = f"{cluster_output_dir}/{dataset_name}/{split}/{video_name}.json"
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        json.dump(video_data, f, indent=4)
    return video_data


def cluster_mask_stage(run, video_path, masks_path, visibility, dataset_name, idmap, video):
    """load_frames_and_masks (crw_utils.py:796-857) + save_segmentation_masks -> (cluster mask dir, {(frame, mask): mask}).
    The frames were decoded for the tracker already; here they give the size the id map is nearest-resized to."""
    frame_num = len(os.listdir(video_path))
    img_paths, lbl_paths = make_paths(video_path, masks_path, dataset_name)
    for i in range(frame_num):
        img_paths[i], lbl_paths[i]                                        # IndexError as in the reference's loop
    H, W = video.shape[-2:]
    ids = idmap.ids
    if (idmap.Hi, idmap.Wi) != (H, W):
        ids = torch.nn.functional.interpolate(ids[:, None].float(), size=(H, W), mode="nearest").long()[:, 0]
    meta = dict(video_path=video_path, img_paths=img_paths, lbl_paths=lbl_paths, visibility=visibility)
    return formats.save_segmentation_masks(None, None, ids, meta, run.args.save_path, return_masks=True)


def _load_cluster_masks(cluster_mask_path, written):
    """load_cluster_masks (cotracker_matching.py:87-128): non-empty cluster_* folders in lexical order, their PNGs in lexical
    order; a mask this run wrote is taken from memory, any other PNG is read"""
    out = []
    for folder in [f for f in sorted(glob.glob(os.path.join(cluster_mask_path, "cluster_*"))) if len(os.listdir(f)) > 0]:
        cid = int(os.path.basename(folder).split("_")[1])
        lst = []
        for mf in sorted(glob.glob(os.path.join(folder, "*.png"))):
            parts = os.path.basename(mf).split("_")
            fid, mid = int(parts[1].replace("frame", "")), int(parts[2].split(".")[0].replace("mask", ""))
            mask = written.get((fid, mid))
            if mask is None:
                try:
                    mask = (np.asarray(Image.open(mf)) > 0).astype(np.uint8) * 255
                except OSError:
                    continue
            lst.append({"vis_cluster_id": cid, "frame_id": fid, "mask_id": mid, "mask": mask})
        out.append(lst)
    return out


def _one2x(all_comparisons):
    """the one-to-many count of :1080-1095: frames in which > 1 object has iou > 0.25; flagged from 5 such frames on"""
    per_frame = {}
    for c in all_comparisons:
        if c["iou"] > 0.25:
            per_frame.setdefault(c["frame_id"], []).append(c["mask_id"])
    return 1 if sum(1 for v in per_frame.values() if len(v) > 1) >= 5 else 0


def _temporal_clustering(matches_data, overall_to_pair):
    """temporal_correspondance_clustering (cotracker_matching.py:764-840) -> mask_groupings, or None for -1"""
    max_id = max([m["overall_mask_id"] for match in matches_data for m in match["matches"]], default=-1)
    out = []
    for cid in sorted(set(m["cluster_id"] for m in matches_data)):
        mat = np.zeros((max_id + 1, max_id + 1), np.float32)
        for match in (m for m in matches_data if int(m["cluster_id"]) == cid):
            ref = match["overall_mask_id"]
            for m in match["matches"]:
                if ref >= mat.shape[0] or m["overall_mask_id"] >= mat.shape[1]:
                    warnings.warn("Overall mask ID exceeds matrix dimensions. Skipping this match.")
                    continue
                mat[ref, m["overall_mask_id"]] = 1
        res = grouping.temporal_groups(mat)
        if res is None:
            return None
        labels, (row_off, _), factor = res
        per_label = {}
        for i, lab in enumerate(labels.tolist()):
            if lab != -1:
                per_label.setdefault(lab, []).append(overall_to_pair[i + row_off])
        out.append({"cluster_id": cid, "visibility_to_temporal_factor": factor, "overall_mask_ids_per_label": per_label})
    return out


def _coverage(cluster_masks, mask_groupings, cluster_mask_path):
    """calculate_cluster_coverage + save_cluster_coverages (cotracker_matching.py:843-872, :434-450)"""
    matched_all = total_all = 0
    covs = []
    for c_masks, grp in zip(cluster_masks, mask_groupings):
        if len(c_masks) == 0:
            continue
        all_c = [(int(m["frame_id"]), int(m["mask_id"])) for m in c_masks]
        matched = sum(1 for m in (m for cm in grp["overall_mask_ids_per_label"].values() for m in cm) if m in all_c)
        covs.append(matched / len(all_c) if len(all_c) > 0 else 0)
        matched_all += matched
        total_all += len(all_c)
    video_cov = matched_all / total_all if total_all > 0 else 0
    with open(os.path.join(cluster_mask_path, "video_coverage.txt"), "w") as f:
        f.write(f"Video Coverage: {video_cov:.2f}\n")
    cids = sorted(int(d.split("_")[1]) for d in os.listdir(cluster_mask_path)
                  if d.startswith("cluster_") and os.path.isdir(os.path.join(cluster_mask_path, d)))
    factors = [m["visibility_to_temporal_factor"] for m in mask_groupings]
    for i, cov in enumerate(covs):
        with open(os.path.join(cluster_mask_path, f"cluster_{cids[i]}", "cluster_coverage.txt"), "w") as f:
            f.write(f"Cluster {cids[i]} Coverage: {cov:.2f}\nVisibility to Temporal Factor: {factors[i]}\n")


def _save_one2x(matches_data, mask_groupings, cluster_mask_path):
    """gather_and_save_one2x_data (cotracker_matching.py:875-923)"""
    per_cluster = {f"cluster_{cid}": [m["one2x"] for m in matches_data if m["cluster_id"] == cid]
                   for cid in sorted(set(m["cluster_id"] for m in matches_data))}
    video = {}
    for grp in mask_groupings:
        cid = grp["cluster_id"]
        gathered = {}
        for g, pairs in grp["overall_mask_ids_per_label"].items():
            gathered[f"group_{g}"] = []
            for fid, mid in pairs:
                v = next((m["one2x"] for m in matches_data if m["frame_id"] == fid and m["mask_id"] == mid), None)
                if v is not None:
                    gathered[f"group_{g}"].append(v)
        out = {"avg_one2x_cluster": np.mean(per_cluster.get(f"cluster_{cid}", []))}
        for name, vals in gathered.items():
            avg = np.sum(vals) / len(vals) if vals else 0
            out[name] = {"avg_one2x": avg, "one2x_counts": len(vals), "noisy": bool(avg > 0.5)}
        with open(os.path.join(cluster_mask_path, f"cluster_{cid}", f"one2x_data_cluster{cid}.json"), "w") as f:
            json.dump(out, f, indent=4)
        video[f"cluster_{cid}"] = out
    with open(os.path.join(cluster_mask_path, "video_one2x_data.json"), "w") as f:
        json.dump(video, f, indent=4)


def matching_stage(run, video_path, cluster_mask_path, written, idmap, video):
    """temporal_correspondence_match (cotracker_matching.py:926-1136) -> 1, or -1 where the reference returns -1"""
    pairs = [(t, int(o)) for t in range(idmap.T) for o in idmap.frame_object_ids(t)]
    overall = {p: i for i, p in enumerate(pairs)}                        # contruct_frameid_maskid_lookup
    cluster_masks = _load_cluster_masks(cluster_mask_path, written)
    if len(cluster_masks) == 0:
        warnings.warn(f"No cluster folders found in {cluster_mask_path!r}. Skipping video!")
        return -1
    cluster_lookup = [{(m["frame_id"], m["mask_id"]): i for i, m in reversed(list(enumerate(c)))} for c in cluster_masks]
    dataset_name, split = stage_dataset(video_path, run.args.dataset_name)
    os.makedirs(os.path.join(run.args.visibility_maps_output_base, dataset_name, split), exist_ok=True)
    video_name = os.path.basename(video_path)
    with open(os.path.join(run.args.visibility_clusters_output_base, dataset_name, split, f"{video_name}.json")) as f:
        clusters = json.load(f)["clusters"]
    clusters.sort(key=lambda x: int(x["cluster_id"]))
    if len(cluster_masks) != len(clusters):
        warnings.warn(f"Cluster masks length {len(cluster_masks)} does not match visibility ranges length {len(clusters)}")
        return -1
    matches_data = []
    idx_correction = 0
    for cl in clusters:
        cid, ranges = cl["cluster_id"], cl["ranges"]
        if len(ranges) == 0:
            if len(cluster_masks) < len(clusters):
                idx_correction += 1
            continue
        v_range = (min(v[0] for v in ranges), max(v[1] for v in ranges))      # merged visibility ranges
        cdata = cluster_masks[cid - idx_correction]
        if len(cdata) == 0:
            continue
        if cdata[0]["vis_cluster_id"] != cid:
            run.log(f"Cluster ID mismatch: {cdata[0]['vis_cluster_id']} != {cid}")
            return -1
        visible = [m for m in cdata if v_range[0] <= m["frame_id"] <= v_range[1]]
        for md in sorted(visible, key=lambda x: int(x["frame_id"])):
            segm, fid, mid = md["mask"], md["frame_id"], md["mask_id"]
            grid_size = max(min(int(np.count_nonzero(segm)) // 800, 50), 25)
            tracks, _ = run.track(video, grid_size, fid, _mask_hw(segm), fid > v_range[0])
            matches, allc = extract_mask_matches_from_tracks(segm.shape, tracks, idmap, v_range, run.args.matching_threshold)
            for rec in matches:
                rec["overall_mask_id"] = overall.get((rec["frame_id"], rec["mask_id"]))
                rec["cluster_mask_id"] = cluster_lookup[cid - idx_correction].get((rec["frame_id"], rec["mask_id"]))
            matches_data.append({"cluster_id": cid, "frame_id": fid, "mask_id": mid, "overall_mask_id": overall.get((fid, mid)),
                                 "cluster_mask_id": cluster_lookup[cid - idx_correction].get((fid, mid)),
                                 "one2x": _one2x(allc), "matches": matches})
    groupings = _temporal_clustering(matches_data, pairs)
    if groupings is None:
        return -1
    formats.save_temporal_group_masks(groupings, cluster_masks, cluster_mask_path, idx_correction)
    _coverage(cluster_masks, groupings, cluster_mask_path)
    _save_one2x(matches_data, groupings, cluster_mask_path)
    return 1


def process_video(run, video_path, masks_path, dataset_name, split):
    """one video through the five stages -> "done" or "failed" (a stage that raises fails the video; the run goes on)"""
    args, name = run.args, os.path.basename(video_path)
    try:
        idmap = load_idmap(masks_path)
        if idmap is None:
            return "failed"
        visibility_data, video = visibility_stage(run, video_path, idmap)
    except Exception as e:
        run.log(f"Error during visibility data extraction for video {name}: {e!r}")
        return "failed"
    if visibility_data is None:
        return "failed"
    try:
        visibility = windows_stage(visibility_data, dataset_name, split, name, args.visibility_clusters_output_base,
                                   args.visibility_threshold)
    except Exception as e:
        run.log(f"Error during visibility window identification for video {name}: {e!r}")
        return "failed"
    try:
        cluster_mask_path, written = cluster_mask_stage(run, video_path, masks_path, visibility, dataset_name, idmap, video)
    except Exception as e:
        run.log(f"Error during segmentation mask saving for video {name}: {e!r}")
        return "failed"
    try:
        status = matching_stage(run, video_path, cluster_mask_path, written, idmap, video)
    except Exception as e:
        run.log(f"Error during temporal correspondence matching for video {name}: {e!r}")
        return "failed"
    if status <= 0:
        run.log(f"No valid annotations found for video: {name}")
        return "failed"
    try:
        formats.write_annotation_for_video(video_path, cluster_mask_path, args.annotation_output_path, visibility)
    except Exception as e:
        run.log(f"Error writing the annotation of video {name}: {e!r}")
        return "failed"
    return "done"


def run(args, tracker=None):
    """the whole discovery run -> the report dict printed as the final JSON line"""
    t0 = time.perf_counter()
    random.seed(args.manualSeed)
    torch.manual_seed(args.manualSeed)
    dataset_name, split = detect_dataset(args.video_base_path, args.dataset_name)
    vids, masks = video_and_mask_dirs(args.video_base_path, args.mask_base_path, args.job_id, args.videos_per_job)
    state = _Run(args, tracker if tracker is not None else load_tracker(args.tracker, args.tracker_checkpoint,
                                                                             parse_tracker_options(args.tracker_options)))
    counts = {"done": 0, "skipped": 0, "failed": 0}
    for video_path, masks_path in zip(vids, masks):
        name = os.path.basename(video_path)
        if os.path.exists(os.path.join(args.annotation_output_path, f"{name}.json")):
            state.log(f"Annotation for video {name} already exists. Skipping.")
            counts["skipped"] += 1
            continue
        state.log("Processing video:", name)
        counts[process_video(state, video_path, masks_path, dataset_name, split)] += 1
    return {"videos": len(vids), **counts, "wall_s": round(time.perf_counter() - t0, 3), "tracker_s": round(state.tracker_s, 3)}


def main(argv=None):
    report = run(parse_args(argv))
    print(json.dumps(report), flush=True)
    return report


if __name__ == "__main__":
    main()
